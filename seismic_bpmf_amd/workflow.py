"""The two detection pipelines around the hot paths, index logic only (no obspy Event objects).

* :func:`matched_filter_detections` = ``MatchedFilter.compute_cc_time_series`` +
  ``find_detections`` / ``_find_detections_t`` (BPMF/similarity_search.py:476-546, 548-666):
  CC on the device, RMS threshold on the device, candidates to the host, the reference's
  pair-wise merge on the (tiny) candidate list.  Returns per-template CC indices.
* :func:`backprojection_detections` = ``Beamformer.backproject`` + ``find_detections``
  (BPMF/template_search.py:508-572, 574-627).
* :func:`intertemplate_cc` = the core of ``TemplateGroup.compute_intertemplate_cc``
  (BPMF/dataset.py:4775-4830).
* :func:`peak_amplitudes` / :func:`detection_aux_data` = the peak amplitudes and the ``aux_data`` that
  ``_find_detections_t`` attaches to every detection (BPMF/similarity_search.py:695-722).
* :func:`templates_from_events` = the templates of the located events, cut from the day on the device
  (``Event.read_waveforms`` + ``Template.init_from_event`` + ``TemplateGroup.normalize``, BPMF/dataset.py).
* :func:`picker_batch` / :func:`resample_poly` / :func:`normalize_batch` / :func:`find_picks` / :func:`pick_events` =
  what surrounds the deep-learning picker in ``Event.pick_PS_phases`` (BPMF/dataset.py:1706-1927;
  ``scipy.signal.resample_poly``, ``utils.normalize_batch``, ``find_picks``, ``get_picks``, BPMF/utils.py:1966-2200):
  device tensors in, device tensors out, pick tables back.
"""
import numpy as np

from . import postprocess as pp
from .beampower import BeamformerGPU
from .matched_filter import MatchedFilterGPU
from .threshold import ThresholdGPU


def _gpu_tensor(name, what, t, definition):
    """The refusal every wrapper of a device entry point opens with; `definition` names what to use on the host."""
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name}: {what} must be a tensor on the GPU (there is no CPU path; {definition})")


def _day(name, data_dev, definition):
    """The refusals of a wrapper that takes the (S, C, N) day in HBM; returns (S, C, N, device)."""
    _gpu_tensor(name, "data_dev", data_dev, definition)
    if data_dev.dim() != 3:
        raise ValueError(f"{name}: data_dev must be (S, C, N)")
    S, Cc, N = (int(v) for v in data_dev.shape)
    return S, Cc, N, data_dev.device


def _window_starts(starts, S):
    """`starts` of a batch of day windows, a tensor or an array, as (E, S) int64 on the host (pp.picker_starts)."""
    import torch
    if isinstance(starts, torch.Tensor):
        starts = starts.detach().cpu().numpy()
    return pp.picker_starts(starts, S)


def _slab_workspace_bytes(need, rows, workspace_bytes, refusal):
    """Bytes of the workspace of an entry point that takes its rows in slabs of a multiple of 64: min(the caller's
    `workspace_bytes`, need(rows)).  ValueError(refusal(workspace_bytes, need(64))) where 64 rows do not fit."""
    workspace_bytes, least = int(workspace_bytes), int(need(64))
    if workspace_bytes < least:
        raise ValueError(refusal(workspace_bytes, least))
    return min(workspace_bytes, int(need(rows)))


def search_window(moveouts_t, minimum_interevent_samp, step):
    """Merge distance between detections of one template, BPMF/similarity_search.py:651-659:
    the median over stations of the moveout spread between components, bounded by 1-10x the
    minimum inter-event time, in CC-step units."""
    d_mv = np.max(moveouts_t, axis=-1) - np.min(moveouts_t, axis=-1)
    d_mv = int(np.median(d_mv)) + 1
    win = min(10 * minimum_interevent_samp, max(d_mv, minimum_interevent_samp))
    return win / step


def search_windows(moveouts, minimum_interevent_samp, step):
    """search_window for every template of a (T, S, C) moveout array at once (same integers)."""
    d_mv = np.max(moveouts, axis=-1) - np.min(moveouts, axis=-1)
    d_mv = np.median(d_mv, axis=-1).astype(np.int64) + 1
    win = np.minimum(10 * minimum_interevent_samp, np.maximum(d_mv, minimum_interevent_samp))
    return win / step


def merge_candidates(index, cc, search_win):
    """The reference's sequential pair-wise merge (BPMF/similarity_search.py:240-251) applied to
    the candidate list: neighbours closer than `search_win` keep only the larger CC."""
    idx = np.asarray(index).tolist()
    val = np.asarray(cc).tolist()
    q = 1
    while q < len(idx):
        if idx[q] - idx[q - 1] < search_win:
            drop = q - 1 if val[q] > val[q - 1] else q
            del idx[drop], val[drop]
        else:
            q += 1
    return np.asarray(idx, dtype=np.int64)


def row_excess_kurtosis(cc):
    """scipy.stats.kurtosis (Fisher, biased: m4 / m2**2 - 3) of every row of a (T, n) float32 device
    tensor, evaluated as SciPy evaluates it on the reference's float32 CC series
    (BPMF/similarity_search.py:633-642): float32 moments in NumPy's summation order
    (csrc/stats.hip, bpmf_row_kurtosis_parts_dev; host mirror postprocess.excess_kurtosis_f32).  Returns a
    float32 NumPy array; NaN for a constant row, like SciPy."""
    import torch
    from . import _lib
    x = cc if cc.dim() == 2 else cc.reshape(1, -1)
    x = x.to(dtype=torch.float32).contiguous()
    rows, n = x.shape
    if rows == 0:
        return np.zeros(0, dtype=np.float32)
    lib = _lib.lib()
    parts = torch.empty((rows, 3), dtype=torch.float32, device=x.device)
    chunk = min(rows, 65535)                   # rows per call of the library (its gridDim.y)
    ws = torch.empty(lib.bpmf_row_kurtosis_workspace_bytes(chunk, n), dtype=torch.uint8, device=x.device)
    for r0 in range(0, rows, chunk):
        _lib.call("bpmf_row_kurtosis_parts_dev", x.device, x[r0:], min(chunk, rows - r0), n, ws, ws.numel(),
                  _lib.STREAM, None, parts[r0:])
    # (mean, m2, m4) per row from the device; the last expression on NumPy scalars, as SciPy evaluates it on one
    # series -- postprocess.kurtosis_from_moments_f32 says why that is not the same as finishing on the device
    from .postprocess import kurtosis_from_moments_rows
    return kurtosis_from_moments_rows(parts.cpu().numpy())


def validation_windows(index, n, win):
    """The two windows MatchedFilter.select_cc_indexes inspects around CC index `index` of a series of n samples
    (BPMF/similarity_search.py:256-263): (start, len_left, len_right) with left = [start, start + len_left) and
    right the len_right samples behind it."""
    half = win // 2
    i0 = np.maximum(0, np.asarray(index, dtype=np.int64) - half)
    i1 = i0 + win
    late = i1 >= n
    i0 = np.where(late, n - 1 - win, i0)
    return i0, half, win - half


def validate_detections(cc, merged, bounds, c_index, c_thr, *, n_dev, threshold_type, cut, win):
    """The anomalous-CDF validation of select_cc_indexes (BPMF/similarity_search.py:253-272) for the merged
    detections {row: cc indices} of a CC matrix in HBM: returns the same dict with the failed detections removed.
    `c_index` / `c_thr` / `bounds`: the candidate arrays of cc_detections (the threshold AT a detection is the
    candidate record's).  Level and fractions as the reference computes them: float32 threshold / n_dev (x 1.48),
    float32 compares, count / float(len) in float64."""
    import torch
    from . import _lib
    n = int(cc.shape[-1])
    if win < 2 or win > n - 1:
        raise ValueError(f"validation window of {win} CC samples on a series of {n}: the reference's slices need "
                         "2 <= int(window_for_validation_Tmax / min_freq_hz) <= n_corr - 1")
    rows, idxs, lvl = [], [], []
    for t, idx in merged.items():
        if len(idx) == 0:
            continue
        b0, b1 = bounds[t], bounds[t + 1]
        pos = b0 + np.searchsorted(c_index[b0:b1], idx)
        one_sigma = c_thr[pos].astype(np.float32) / np.float32(n_dev)
        if threshold_type == "mad":
            one_sigma = one_sigma * np.float32(1.48)
        rows.append(np.full(len(idx), t, dtype=np.int32))
        idxs.append(np.asarray(idx, dtype=np.int64))
        lvl.append(one_sigma.astype(np.float32))
    if not rows:
        return merged
    rows, idxs, lvl = np.concatenate(rows), np.concatenate(idxs), np.concatenate(lvl)
    start, n_left, n_right = validation_windows(idxs, n, win)
    dev = cc.device
    d_rows = torch.as_tensor(rows, device=dev)
    d_start = torch.as_tensor(start.astype(np.int64), device=dev)
    d_nl = torch.full((len(rows),), n_left, dtype=torch.int32, device=dev)
    d_nr = torch.full((len(rows),), n_right, dtype=torch.int32, device=dev)
    d_lvl = torch.as_tensor(lvl, device=dev)
    below = torch.empty((len(rows), 2), dtype=torch.int32, device=dev)
    x = cc if cc.is_contiguous() else cc.contiguous()
    _lib.call("bpmf_count_below_dev", dev, x, int(x.shape[0]), n, len(rows), d_rows, d_start, d_nl, d_nr, d_lvl,
              _lib.STREAM, below)
    below = below.cpu().numpy().astype(np.float64)
    frac = np.minimum(below[:, 0] / float(n_left), below[:, 1] / float(n_right))
    keep = ~(frac < cut)
    out = dict(merged)
    for t in np.unique(rows):
        m = rows == t
        out[int(t)] = idxs[m][keep[m]]
    return out


def peak_amplitudes(data_dev, rows, samples, moveouts, *, offset, duration, data_norm=None):
    """The peak amplitudes of ``MatchedFilter._find_detections_t`` (BPMF/similarity_search.py:695-714) for the
    detections of ALL templates in one launch (bpmf_peak_amplitudes_dev, csrc/peak_amp.hip): out[q, s, c] is the
    maximum of data[s, c, i1:i2], i1 = samples[q] + moveouts[rows[q], s, c] - offset, i2 = i1 + duration -- the
    reference's own NumPy slice, see postprocess.peak_amplitudes_host -- times data_norm[s, c]; 0.0 for an empty
    window.

    `data_dev`: the (S, C, N) float32 day as a tensor on the GPU (what MatchedFilterGPU.data holds); `rows` (D,)
    template rows; `samples` (D,) DATA samples (cc index x step); `moveouts` (T, S[, C]) in samples -- per component
    the moveout of the phase the reference's `phase_on_comp_peak_amp` names; `offset` / `duration` in samples;
    `data_norm` (S, C) or None.  Uploads the detection records and the moveout table, downloads D * S * C floats.
    Returns a (D, S, C) float32 NumPy array."""
    import torch
    from . import _lib
    S, Cc, N, dev = _day("peak_amplitudes", data_dev, "the host mirror is postprocess.peak_amplitudes_host")
    x = data_dev.to(dtype=torch.float32).contiguous()
    rows = np.ascontiguousarray(np.asarray(rows).reshape(-1), dtype=np.int32)
    samples = np.ascontiguousarray(np.asarray(samples).reshape(-1), dtype=np.int64)
    if rows.shape != samples.shape:
        raise ValueError("peak_amplitudes: rows and samples must have one entry per detection")
    mv = moveouts.detach().cpu().numpy() if isinstance(moveouts, torch.Tensor) else np.asarray(moveouts)
    if mv.ndim not in (2, 3) or mv.shape[1] != S or (mv.ndim == 3 and mv.shape[2] not in (1, Cc)):
        raise ValueError(f"peak_amplitudes: moveouts must be (T, {S}) or (T, {S}, {Cc}); got {mv.shape}")
    T = int(mv.shape[0])
    mv = np.array(np.broadcast_to(mv.reshape(T, S, -1), (T, S, Cc)), dtype=np.int32, order="C")
    norm = None
    if data_norm is not None:
        norm = np.ascontiguousarray(data_norm, dtype=np.float32)
        if norm.shape != (S, Cc):
            raise ValueError(f"peak_amplitudes: data_norm must be ({S}, {Cc}); got {norm.shape}")
    D = len(rows)
    if D == 0:
        return np.zeros((0, S, Cc), dtype=np.float32)
    d_rows = torch.as_tensor(rows, device=dev)
    d_samples = torch.as_tensor(samples, device=dev)
    d_mv = torch.as_tensor(mv, device=dev)
    d_norm = None if norm is None else torch.as_tensor(norm, device=dev)
    out = torch.empty((D, S, Cc), dtype=torch.float32, device=dev)
    _lib.call("bpmf_peak_amplitudes_dev", dev, x, S, Cc, N, D, d_rows, d_samples, d_mv, T, int(offset), int(duration),
              d_norm, _lib.STREAM, out)
    return out.cpu().numpy()


def templates_from_events(data_dev, origin_samples, moveouts, n_samples, *, normalize="rms", noise_offset=None,
                          noise_samples=None, min_channels=6, min_stations=3, require_complete=True):
    """Matched-filter templates cut from the day in HBM at the located events, all events in one launch
    (bpmf_templates_from_events_dev, csrc/templates.hip) -- what Event.read_waveforms(time_shifted=True),
    Template.init_from_event / set_availability, TemplateGroup.normalize and Event.compute_snr do array by array on
    the host (BPMF/dataset.py:1929-2069, 3322-3405, 2556-2607, 4152-4166, 1441-1475).  The definition, with its two
    stated departures from the reference, is postprocess.templates_from_events_host; the device equals it bit for bit.

    `data_dev`: the (S, C, N) float32 day as a tensor on the GPU (what MatchedFilterGPU.data holds);
    `origin_samples` (E,) int64; `moveouts` (E, S[, C]) int32 WINDOW moveouts (postprocess.template_window_moveouts);
    `n_samples` 1 .. 8192; `normalize` "rms" | "max" | None; `noise_offset` / `noise_samples` (samples; up to 8192):
    the noise window of the SNR, none by default.

    Returns a dict.  On the day's device, as MatchedFilterGPU.run(templates, moveouts, weights) takes them:
    `templates` (E, S, C, L) float32, `moveouts` (E, S, C) int32, `weights` (E, S, C) float32 =
    normalize_weights(weights_channels_simple(available [& complete when `require_complete`], min_channels,
    min_stations)).  On the host: `available`, `complete` (E, S, C) bool, `norm` (E, S, C) float32, `snr` (E, S, C)
    float32 or None."""
    import torch
    from . import _lib
    S, Cc, N, dev = _day("templates_from_events", data_dev,
                         "the definition on the host is postprocess.templates_from_events_host")
    if isinstance(moveouts, torch.Tensor):
        moveouts = moveouts.detach().cpu().numpy()
    if isinstance(origin_samples, torch.Tensor):
        origin_samples = origin_samples.detach().cpu().numpy()
    origin, mv, L, n_noise, offset = pp.template_arguments(S, Cc, origin_samples, moveouts, n_samples, normalize,
                                                           noise_offset, noise_samples)
    if N == 0:
        raise ValueError("templates_from_events: the day is empty")
    E = len(origin)
    with torch.cuda.device(dev):
        x = data_dev.to(dtype=torch.float32).contiguous()
        d_mv = torch.as_tensor(mv, device=dev)
        templates = torch.empty((E, S, Cc, L), dtype=torch.float32, device=dev)
        norm = torch.empty((E, S, Cc), dtype=torch.float32, device=dev)
        flags = torch.empty((E, S, Cc), dtype=torch.uint8, device=dev)
        snr = torch.empty((E, S, Cc), dtype=torch.float32, device=dev) if n_noise else None
        if E:
            d_origin = torch.as_tensor(origin, device=dev)
            _lib.call("bpmf_templates_from_events_dev", dev, x, S, Cc, N, E, d_origin, d_mv, L,
                      {None: 0, "rms": 1, "max": 2}[normalize], offset, n_noise, _lib.STREAM, templates, norm, flags, snr)
        flags_host = flags.cpu().numpy()
        available, complete = (flags_host & 1) != 0, (flags_host & 2) != 0
        present = available & complete if require_complete else available
        weights = pp.normalize_weights(pp.weights_channels_simple(present, min_channels, min_stations))
        return {"templates": templates, "moveouts": d_mv, "weights": torch.as_tensor(weights, device=dev),
                "available": available, "complete": complete, "norm": norm.cpu().numpy(),
                "snr": None if snr is None else snr.cpu().numpy()}


NORMALIZE_BATCH_LDS_FLOATS = 38400           # n + 2 shift + W + 2 n_windows of one row (csrc/picker.hip)
FIND_PICKS_MAX_SAMPLES = 16384
FIND_PICKS_MAX_PICKS = 4096


def _normalize_checks(what, shape, n_rows, n, W, overlap, dtype):
    """The refusals of the normalisation of `n_rows` rows of `n` samples cut from an (S, C, N) tensor; returns
    (shift, n_windows)."""
    import torch
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what}: dtype must be torch.float32 or torch.float64; got {dtype}")
    S, Cc, N = shape
    shift, n_windows = pp.normalize_batch_plan(n, normalization_window_sample=W, overlap=overlap)
    floats = n + 2 * shift + int(W) + 2 * n_windows
    if floats > NORMALIZE_BATCH_LDS_FLOATS:
        raise ValueError(f"{what}: a row of {n} samples with windows of {int(W)} at shift {shift} takes {floats} floats "
                         f"of LDS; at most {NORMALIZE_BATCH_LDS_FLOATS} fit")
    if S * Cc == 0 or N == 0:
        raise ValueError(f"{what}: the data are empty")
    if n_rows * Cc >= 2**31:
        raise ValueError(f"{what}: {n_rows} x {Cc} rows in one call; fewer than 2^31 fit")
    return shift, n_windows


def _normalize_rows(what, x, n_rows, d_start, n, W, overlap, dtype, out_shape):
    """Checks on the host, then one bpmf_normalize_batch_dev launch on the current stream of x's device: rows
    (r, c) = x[r % S, c, start[r] + i] of the contiguous float32 (S, C, N) tensor `x`."""
    import torch
    from . import _lib
    S, Cc, N = (int(v) for v in x.shape)
    shift, n_windows = _normalize_checks(what, (S, Cc, N), n_rows, n, W, overlap, dtype)
    dev = x.device
    with torch.cuda.device(dev):
        out = torch.empty(out_shape, dtype=dtype, device=dev)
        if n_rows == 0:
            return out
        nodes = torch.as_tensor(pp.normalize_batch_nodes(n, shift, n_windows), device=dev)
        _lib.call("bpmf_normalize_batch_dev", dev, x, S, Cc, N, n_rows, d_start, n, int(W), shift, nodes, n_windows,
                  int(dtype == torch.float64), _lib.STREAM, out)
    return out


def normalize_batch(x_dev, normalization_window_sample=3000, overlap=0.5, dtype=None):
    """utils.normalize_batch (BPMF/utils.py:1966-2036), the running Z-score in front of the deep-learning picker, of an
    already cut (R, C, n) float32 tensor on the GPU, in one launch (bpmf_normalize_batch_dev, csrc/picker.hip) on the
    current stream.  Returns a tensor on the same device: float32 by default (the `.float()` of the reference's
    float64 result, as the tutorial's ml_picker takes it) or, with dtype=torch.float64, the float64 result itself.  The
    definition is postprocess.normalize_batch_host, which equals the reference bit for bit; the device equals it bit
    for bit, NaN samples included.  Refusals (ValueError, before any device call): a window under 2 or over 8192
    samples, a shift int((1 - overlap) * W) under 1 or over n - 1, fewer than two windows, a row too long for LDS
    (n + 2 shift + W + 2 n_windows over 38400: n = 16384 with W = 3000 takes 22406).

    The resample_poly up- and down-sampling that Event.pick_PS_phases runs in front of it is resample_poly below (and
    picker_batch(upsampling=, downsampling=) runs both on the windows of a day).  Out of scope: the model itself; the
    power-of-two reflect padding of tutorial/notebooks/6_relocate.ipynb cell 54; infinite samples."""
    import torch
    _gpu_tensor("normalize_batch", "x_dev", x_dev, "the definition on the host is postprocess.normalize_batch_host")
    if x_dev.dim() != 3:
        raise ValueError("normalize_batch: x_dev must be (R, C, n)")
    R, Cc, n = (int(v) for v in x_dev.shape)
    with torch.cuda.device(x_dev.device):
        x = x_dev.to(dtype=torch.float32).contiguous()
    return _normalize_rows("normalize_batch", x, R, None, n, normalization_window_sample, overlap,
                           torch.float32 if dtype is None else dtype, (R, Cc, n))


def _resample_checks(what, shape, n_rows, n_in, up, down):
    """The refusals of the resampling of `n_rows` rows of `n_in` samples cut from an (S, C, N) tensor by the reduced
    up / down; returns (n_out, n_pre_remove, table, hp) of postprocess.resample_poly_plan."""
    S, Cc, N = shape
    _, n_out, _, n_pre_remove, _, table = pp.resample_poly_plan(n_in, up, down)
    hp = len(table) // up
    if S * Cc == 0 or N == 0:
        raise ValueError(f"{what}: the data are empty")
    if n_rows * Cc >= 2**31:
        raise ValueError(f"{what}: {n_rows} x {Cc} rows in one call; fewer than 2^31 fit")
    tile = resample_poly_tile(up, down, hp)
    if n_rows * Cc * (-(-n_out // tile)) >= 2**31:
        raise ValueError(f"{what}: {n_rows * Cc} rows of {n_out} output samples take 2^31 tiles of {tile} or more")
    return n_out, n_pre_remove, table, hp


def _resample_rows(what, x, n_rows, d_start, n_in, up, down):
    """Checks on the host, then one bpmf_resample_poly_dev launch on the current stream of x's device: rows
    (r, c) = x[r % S, c, start[r] + i], i < n_in, of the contiguous float32 (S, C, N) tensor `x`, resampled by the
    reduced up / down (not both 1).  Returns (n_rows, C, n_out) float32."""
    import torch
    from . import _lib
    S, Cc, N = (int(v) for v in x.shape)
    n_out, n_pre_remove, table, hp = _resample_checks(what, (S, Cc, N), n_rows, n_in, up, down)
    dev = x.device
    with torch.cuda.device(dev):
        out = torch.empty((n_rows, Cc, n_out), dtype=torch.float32, device=dev)
        if n_rows == 0:
            return out
        d_table = torch.as_tensor(table, device=dev)
        _lib.call("bpmf_resample_poly_dev", dev, x, S, Cc, N, n_rows, d_start, n_in, up, down, d_table, hp,
                  n_pre_remove, n_out, _lib.STREAM, out)
    return out


def resample_poly_tile(up, down, taps_per_phase):
    """The output samples one workgroup of bpmf_resample_poly_dev makes (csrc/resample.hip picks it so that the tap
    table and the tile's input span fit its LDS budget): a row of n_out samples takes ceil(n_out / tile) workgroups."""
    from . import _lib
    tile = int(_lib.lib().bpmf_resample_poly_tile(int(up), int(down), int(taps_per_phase)))
    if tile == 0:
        raise ValueError(f"resample_poly: no tile for up={up} down={down} taps_per_phase={taps_per_phase}")
    return tile


def resample_poly(x_dev, up, down):
    """scipy.signal.resample_poly(x, up, down, axis=-1) (default window and padtype) of a (..., n) float32 tensor on the
    GPU, in one launch (bpmf_resample_poly_dev, csrc/resample.hip) on the current stream: the up- and down-sampling
    that Event.pick_PS_phases(upsampling=, downsampling=) runs between cutting the windows and normalising them
    (BPMF/dataset.py:1801-1804; 5596-5599 in Stack.pick_PS_phases_family_mode).  Returns (..., n_out) float32 on the
    same device, n_out = ceil(n up / down).  The definition is postprocess.resample_poly_host, which equals SciPy bit
    for bit; the device equals it bit for bit, NaN samples included.  up == down after the reduction by their gcd
    returns a copy.  Refusals (ValueError, before any device call): factors that are no integers or under 1, a
    reduced max(up, down) over 64, n < 1, n max(up, down) >= 2^40, a dtype other than float32.

    Out of scope: the other `padtype` and `window` arguments; float64 and complex input."""
    import torch
    _gpu_tensor("resample_poly", "x_dev", x_dev, "the definition on the host is postprocess.resample_poly_host")
    if x_dev.dim() < 1 or x_dev.dtype != torch.float32:
        raise ValueError(f"resample_poly: x_dev must be (..., n) float32; got {x_dev.dtype} {tuple(x_dev.shape)}")
    up, down = pp.resample_poly_factors(up, down)
    lead, n = tuple(int(v) for v in x_dev.shape[:-1]), int(x_dev.shape[-1])
    n_out = pp.resample_poly_plan(n, up, down)[1]
    R = int(np.prod(lead, dtype=np.int64))
    if up != down and R:
        _resample_checks("resample_poly", (R, 1, n), R, n, up, down)
    with torch.cuda.device(x_dev.device):
        if up == down:
            return x_dev.clone(memory_format=torch.contiguous_format)
        if R == 0:
            return torch.empty(lead + (n_out,), dtype=torch.float32, device=x_dev.device)
        x = x_dev.contiguous().view(R, 1, n)
    return _resample_rows("resample_poly", x, R, None, n, up, down).view(lead + (n_out,))


def picker_batch(data_dev, starts, n_samples, *, normalization_window_sample=3000, overlap=0.5, dtype=None,
                 upsampling=1, downsampling=1):
    """The picker's input batch for E events, cut from the day in HBM and normalised in one launch
    (bpmf_normalize_batch_dev, csrc/picker.hip): out[e, s, c, :] = normalize_batch of the window
    data[s, c, starts[e(, s)] : + n_samples], zero-padded where it leaves the day -- what Event.read_waveforms +
    utils.get_np_array + utils.normalize_batch make on the host for every event (BPMF/dataset.py:1770-1810,
    BPMF/utils.py:1966-2036) -- without the un-normalised windows ever being stored.  Bit for bit
    normalize_batch(the zero-padded cut windows) (postprocess.picker_windows_host / normalize_batch_host).

    `data_dev`: the (S, C, N) float32 day as a tensor on the GPU (what MatchedFilterGPU.data holds); `starts` (E,) or
    (E, S) int64 window starts in samples (origin - offset_ot), any sign, within +-2^40; `n_samples` per window.
    Returns (E, S, C, n_samples) on the day's device and the current stream, float32 by default, ready for
    model(x.flatten(0, 1)).  DEPARTURE: a window cut by the START of the day keeps its alignment here (zeros in
    front); the reference left-aligns the samples it could read and pads behind them.

    `upsampling` / `downsampling`: the keywords of Event.pick_PS_phases for data that are not at the picker's rate
    (the tutorial's 25 Hz day and a 100 Hz picker: upsampling=4).  The windows of `n_samples` INPUT samples are then
    resampled between the cut and the normalisation, as BPMF/dataset.py:1801-1804 does with scipy.signal.resample_poly:
    bpmf_resample_poly_dev (csrc/resample.hip) writes the resampled windows to a temporary (E S, C, n_out) tensor and
    bpmf_normalize_batch_dev normalises it.  Returns (E, S, C, n_out), n_out = ceil(n_samples up / down): bit for bit
    normalize_batch_host(resample_poly_host(picker_windows_host(...))).  The normalisation window and its refusals then
    count in RESAMPLED samples, and so do the picks that find_picks / pick_events make of the model's output.  Equal
    factors (1 and 1 after the reduction by their gcd) take the path without resampling: the same launch and bits.

    Refusals (every one before any device call) and what is out of scope: see normalize_batch and resample_poly."""
    import torch
    S, Cc, N, dev = _day("picker_batch", data_dev, "the definition on the host is postprocess.normalize_batch_host of "
                                                   "postprocess.picker_windows_host")
    st = _window_starts(starts, S)
    n = int(n_samples)
    up, down = pp.resample_poly_factors(upsampling, downsampling)
    dtype = torch.float32 if dtype is None else dtype
    W = normalization_window_sample
    n_out = n
    if up != down:
        n_out = _resample_checks("picker_batch", (S, Cc, N), st.size, n, up, down)[0]
        _normalize_checks("picker_batch", (S, Cc, N), st.size, n_out, W, overlap, dtype)
    with torch.cuda.device(dev):
        x = data_dev.to(dtype=torch.float32).contiguous()
        d_start = torch.as_tensor(st.reshape(-1), device=dev) if st.size else None
    if up != down:
        if st.size == 0:
            return torch.empty((0, S, Cc, n_out), dtype=dtype, device=dev)
        resampled = _resample_rows("picker_batch", x, st.size, d_start, n, up, down)
        return _normalize_rows("picker_batch", resampled, st.size, None, n_out, W, overlap, dtype,
                               (len(st), S, Cc, n_out))
    return _normalize_rows("picker_batch", x, st.size, d_start, n, W, overlap, dtype, (len(st), S, Cc, n))


def find_picks(proba_dev, threshold_P=0.6, threshold_S=0.6, max_picks=32, truncate=False):
    """utils.find_picks (BPMF/utils.py:2039-2094, default keywords) on every series of the picker's output while it
    is still on the GPU, in one launch (bpmf_find_picks_dev, csrc/picker.hip): only the pick tables leave the device.
    `proba_dev` (..., 2, n) float32 on the GPU, [..., 0, :] the P and [..., 1, :] the S probabilities, n <= 16384.
    Returns a dict of host arrays: `count` (..., 2) int32, the number of picks of each series; `value` float32 (the
    probability at the peak), `mean`, `std` float64 (the pick and its spread, in samples) and `index` int32 (the peak
    sample), each (..., 2, max_picks), ascending in time, NaN / -1 in the unused slots.  The definition is
    postprocess.find_picks_host; the device equals it bit for bit.  A series with more than `max_picks` picks raises
    RuntimeError, unless `truncate`: then its first max_picks picks are kept and `count` tells how many there were.

    Out of scope: find_peaks keywords other than the reference's defaults; infinite samples."""
    import torch
    from . import _lib
    _gpu_tensor("find_picks", "proba_dev", proba_dev, "the definition on the host is postprocess.find_picks_host")
    if proba_dev.dim() < 2 or proba_dev.shape[-2] != 2:
        raise ValueError(f"find_picks: proba_dev must be (..., 2, n); got {tuple(proba_dev.shape)}")
    n, max_picks = int(proba_dev.shape[-1]), int(max_picks)
    if not 1 <= n <= FIND_PICKS_MAX_SAMPLES:
        raise ValueError(f"find_picks: series of 1 .. {FIND_PICKS_MAX_SAMPLES} samples; got {n}")
    if not 1 <= max_picks <= FIND_PICKS_MAX_PICKS:
        raise ValueError(f"find_picks: max_picks must be 1 .. {FIND_PICKS_MAX_PICKS}; got {max_picks}")
    thresholds = (float(threshold_P), float(threshold_S))
    if any(t != t for t in thresholds):
        raise ValueError("find_picks: the thresholds must be numbers")
    lead = tuple(int(v) for v in proba_dev.shape[:-1])
    T = int(np.prod(lead))
    if T >= 2**31:
        raise ValueError("find_picks: fewer than 2^31 series in one call")
    dev = proba_dev.device
    with torch.cuda.device(dev):
        x = proba_dev.to(dtype=torch.float32).contiguous()
        count = torch.empty(lead, dtype=torch.int32, device=dev)
        value = torch.empty(lead + (max_picks,), dtype=torch.float32, device=dev)
        mean = torch.empty(lead + (max_picks,), dtype=torch.float64, device=dev)
        std = torch.empty(lead + (max_picks,), dtype=torch.float64, device=dev)
        index = torch.empty(lead + (max_picks,), dtype=torch.int32, device=dev)
        if T:
            _lib.call("bpmf_find_picks_dev", dev, x, T, n, thresholds[0], thresholds[1], max_picks, _lib.STREAM, count,
                      value, mean, std, index)
        out = {"count": count.cpu().numpy(), "value": value.cpu().numpy(), "mean": mean.cpu().numpy(),
               "std": std.cpu().numpy(), "index": index.cpu().numpy()}
    if not truncate and T and out["count"].max() > max_picks:
        raise RuntimeError(f"find_picks: a series holds {int(out['count'].max())} picks, more than max_picks = "
                           f"{max_picks}; raise max_picks or pass truncate=True")
    return out


def pick_events(proba_dev, *, threshold_P, threshold_S, buffer_length, prior=None, search_win_samp=None, sr=None,
                max_picks=32):
    """One P and one S pick per station for E events, from the picker's (E, S, 2, n) probabilities on the GPU:
    find_picks on the device, then postprocess.get_picks_host (utils.get_picks, BPMF/utils.py:2097-2200) per event on
    the small pick tables -- the second half of Event.pick_PS_phases (BPMF/dataset.py:1854-1898).  `buffer_length`
    (samples): picks up to it are discarded (the reference binds int(2 * cfg.SAMPLING_RATE_HZ) at import time);
    `prior` (S, 2) or (E, S, 2): a priori P and S picks in samples, NaN rows for stations without one, with
    `search_win_samp`.  Returns (E, S, 6) float32 in the order of postprocess.PICK_COLUMNS, NaN where there is no pick:
    picks and uncertainties in samples, or in seconds when `sr` is given (the division of :1895-1898).  Behind
    picker_batch(upsampling=, downsampling=) the samples are those of the RESAMPLED rate: `sr` is then
    sr * upsampling / downsampling, as BPMF/dataset.py:1807 sets it, and so are buffer_length, prior and search_win_samp.

    Out of scope: absolute pick times and the pandas table; see find_picks and normalize_batch for the rest."""
    _gpu_tensor("pick_events", "proba_dev", proba_dev,
                "the definitions on the host are postprocess.find_picks_host and postprocess.get_picks_host")
    if proba_dev.dim() != 4 or proba_dev.shape[2] != 2:
        raise ValueError(f"pick_events: proba_dev must be (E, S, 2, n); got {tuple(proba_dev.shape)}")
    E, S = int(proba_dev.shape[0]), int(proba_dev.shape[1])
    if prior is not None:
        prior = np.asarray(prior, dtype=np.float64)
        if prior.shape not in ((S, 2), (E, S, 2)):
            raise ValueError(f"pick_events: prior must be ({S}, 2) or ({E}, {S}, 2); got {prior.shape}")
        if search_win_samp is None:
            raise ValueError("pick_events: prior needs search_win_samp")
        prior = np.broadcast_to(prior, (E, S, 2))
    picks = find_picks(proba_dev, threshold_P, threshold_S, max_picks=max_picks)
    out = np.full((E, S, 6), np.nan, dtype=np.float32)
    for e in range(E):
        out[e] = pp.get_picks_host(picks["value"][e], picks["mean"][e], picks["std"][e], picks["count"][e],
                                   buffer_length, None if prior is None else prior[e], search_win_samp)
    if sr is not None:
        out[..., [1, 2, 4, 5]] = out[..., [1, 2, 4, 5]] / np.float32(sr)
    return out


SVDWF_WORKSPACE_BYTES = 2 << 30            # svdwf_stack: the workspace it asks for at most (and at least one channel)


def bandpass_filter(x_dev, sos=None, *, freqmin=None, freqmax=None, f_Nyq=None, filter_order=4, detrend=True,
                    taper_alpha=0.01, zerophase=True, dtype=None):
    """utils.bandpass_filter (BPMF/utils.py:24-90) along the last axis of any (..., m) float32 or float64 tensor on the
    GPU, one launch on the current stream (bpmf_bandpass_rows_dev, csrc/svdwf.hip): mean and least-squares line removed
    (`detrend`), Tukey taper (`taper_alpha`, None for none), the Butterworth band-pass `filter_order` corners between
    `freqmin` and `freqmax` (postprocess.butter_bandpass_sos) or the caller's `sos` (n_sections <= 8, 6) table, forward
    and -- `zerophase` -- backward, from zero state, in float64.  Returns a tensor of the same shape and device,
    float64 by default as the reference returns it, or `dtype` torch.float32.  The definition is
    postprocess.bandpass_filter_host; without detrend and taper the float64 result equals it (and SciPy's sosfilt) bit
    for bit."""
    import torch
    from . import _lib
    _gpu_tensor("bandpass_filter", "x_dev", x_dev, "the definition on the host is postprocess.bandpass_filter_host")
    if x_dev.dim() < 1 or x_dev.dtype not in (torch.float32, torch.float64):
        raise ValueError("bandpass_filter: x_dev must be a float32 or float64 tensor (..., m)")
    dtype = torch.float64 if dtype is None else dtype
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"bandpass_filter: dtype must be torch.float32 or torch.float64; got {dtype}")
    table = pp.bandpass_sos(sos, freqmin, freqmax, f_Nyq, filter_order)
    alpha = -1.0 if taper_alpha is None else float(taper_alpha)
    if alpha != alpha:
        raise ValueError("bandpass_filter: taper_alpha must be a number or None")
    m = int(x_dev.shape[-1])
    rows = int(np.prod(x_dev.shape[:-1]))
    if m == 0 or m > 2**24 or rows >= 2**31:
        raise ValueError(f"bandpass_filter: rows of 1 .. 2^24 samples, fewer than 2^31 of them; got {rows} x {m}")
    dev = x_dev.device
    with torch.cuda.device(dev):
        x = x_dev.contiguous()
        out = torch.empty(x.shape, dtype=dtype, device=dev)
        if rows == 0:
            return out
        d_sos = torch.as_tensor(table, device=dev)
        out_f64, zp = int(dtype == torch.float64), int(bool(zerophase))
        need = _lib.lib().bpmf_bandpass_rows_workspace_bytes(rows, m, zp, out_f64)
        ws = torch.empty((need,), dtype=torch.uint8, device=dev) if need else None
        _lib.call("bpmf_bandpass_rows_dev", dev, x, int(x.dtype == torch.float64), rows, m, d_sos, table.shape[0],
                  int(bool(detrend)), alpha, zp, out_f64, ws, need, _lib.STREAM, out)
    return out


def svdwf_stack(x_dev, offsets=None, *, expl_var=0.4, max_singular_values=5, wiener_filter_colsize=None,
                freqmin=None, freqmax=None, sampling_rate=None, sos=None, taper_alpha=0.01, return_filtered=True,
                strict=True, workspace=None):
    """EventGroup.SVDWF_stack (BPMF/dataset.py:4275-4374; utils.SVDWF, BPMF/utils.py:667-772) for a ragged batch of
    templates in one call (bpmf_svdwf_stack_dev, csrc/svdwf.hip): the SVD-Wiener filter of every channel's (n, m)
    matrix of detections, the band-pass behind it, the mean over the events and its normalisation by the signed
    maximum -- the stack that becomes the template of the next iteration.

    `x_dev` (N, S, C, m) float32 on the GPU: the waveforms of all detections (what templates_from_events cuts),
    group g = rows offsets[g] .. offsets[g + 1] (`offsets` (G + 1,) ascending from 0 to N; None: one group).  A group
    holds at most 512 events of up to 16384 samples, or up to 16384 events of at most 512 samples.  The band-pass is
    applied when `sampling_rate` is given (order 4 between `freqmin` and `freqmax`, as the reference) or with a
    caller's `sos` table; `wiener_filter_colsize` None: each group's size.

    Returns (stack, filtered, n_singular, status): `stack` (G, S, C, m) float32 and `filtered` (N, S, C, m) float32
    (None without `return_filtered`) on x_dev's device, `n_singular` (G, S, C) int32 (0 for a zero channel) and `status`
    (G, S, C) int32 on the host.  A channel whose eigen-solve did not converge (status 1; its outputs are zeros)
    raises RuntimeError unless strict=False.  The definition is postprocess.svdwf_stack_host, within 2^-22 of each
    channel's largest |filtered| and 2^-21 on the stack.  `workspace`: a uint8 tensor to work in (at
    least one channel's worth, bpmf_svdwf_workspace_bytes); by default up to 2 GiB are allocated for the call.

    Departure: where LAPACK fails the reference returns Gaussian noise; here `status` reports it.  A channel that
    holds a NaN or an Inf is not solved: it has status 1 and zero outputs, and every other channel of the batch has
    the bits it has without it.  Out of scope: fetching the waveforms, the Stack object."""
    import ctypes as C
    import torch
    from . import _lib
    _gpu_tensor("svdwf_stack", "x_dev", x_dev, "the definition on the host is postprocess.svdwf_stack_host")
    if x_dev.dim() != 4:
        raise ValueError("svdwf_stack: x_dev must be (N, S, C, m)")
    N, S, Cc, m = (int(v) for v in x_dev.shape)
    if isinstance(offsets, torch.Tensor):
        offsets = offsets.detach().cpu().numpy()
    off = pp.group_offsets(N, offsets)
    G = len(off) - 1
    expl_var, kmax, w = pp.svdwf_arguments(N, m, expl_var, max_singular_values, wiener_filter_colsize)
    if S * Cc == 0:
        raise ValueError("svdwf_stack: the waveforms hold no channels")
    sizes = np.diff(off)
    n_max = int(sizes.max()) if G else 0
    if G and (np.minimum(sizes, m).max() > pp.SVDWF_MAX_SMALL_SIDE or max(n_max, m) > pp.SVDWF_MAX_LARGE_SIDE):
        raise ValueError(f"svdwf_stack: a group of {n_max} events x {m} samples is not served: min(n, m) <= "
                         f"{pp.SVDWF_MAX_SMALL_SIDE} and max(n, m) <= {pp.SVDWF_MAX_LARGE_SIDE}")
    if w is not None and w > 65536:
        raise ValueError(f"svdwf_stack: wiener_filter_colsize <= 65536; got {w}")
    if max(N, G) * S * Cc >= 2**31:
        raise ValueError("svdwf_stack: fewer than 2^31 rows in one call")
    table = None
    if sos is not None or sampling_rate is not None:
        table = pp.bandpass_sos(sos, freqmin, freqmax, None if sampling_rate is None else float(sampling_rate) / 2.0, 4)
    alpha = -1.0 if taper_alpha is None else float(taper_alpha)
    dev = x_dev.device
    with torch.cuda.device(dev):
        x = x_dev.to(dtype=torch.float32).contiguous()
        stack = torch.empty((G, S, Cc, m), dtype=torch.float32, device=dev)
        filtered = torch.empty((N, S, Cc, m), dtype=torch.float32, device=dev) if return_filtered else None
        n_singular = torch.empty((G, S, Cc), dtype=torch.int32, device=dev)
        status = torch.empty((G, S, Cc), dtype=torch.int32, device=dev)
        if G:
            lib = _lib.lib()
            if workspace is None:
                one = lib.bpmf_svdwf_workspace_bytes(G, n_max, m, 1)
                per = one - lib.bpmf_svdwf_workspace_bytes(G, n_max, m, 0)
                channels = max(1, min(G * S * Cc, SVDWF_WORKSPACE_BYTES // max(per, 1)))
                workspace = torch.empty((lib.bpmf_svdwf_workspace_bytes(G, n_max, m, channels),), dtype=torch.uint8,
                                        device=dev)
            elif not (isinstance(workspace, torch.Tensor) and workspace.is_cuda and workspace.dtype == torch.uint8
                      and workspace.is_contiguous() and workspace.data_ptr() % 256 == 0):
                raise ValueError("svdwf_stack: workspace must be a contiguous uint8 tensor on the GPU, aligned to 256")
            d_sos = None if table is None else torch.as_tensor(table, device=dev)
            _lib.call("bpmf_svdwf_stack_dev", dev, x, off.ctypes.data_as(C.POINTER(C.c_int64)), G, S, Cc, m, expl_var,
                      kmax, 0 if w is None else w, d_sos, 0 if table is None else table.shape[0], alpha, workspace,
                      int(workspace.numel()), _lib.STREAM, filtered, stack, n_singular, status)
        n_singular, status = n_singular.cpu().numpy(), status.cpu().numpy()
    if strict and status.any():
        bad = np.argwhere(status != 0)[0]
        raise RuntimeError(f"svdwf_stack: the eigen-solve of {int((status != 0).sum())} channel(s) did not converge, "
                           f"or the channel holds a NaN or an Inf (first: group {bad[0]}, station {bad[1]}, component {bad[2]}); pass strict=False to get "
                           "zeros there and the status array")
    return stack, filtered, n_singular, status


MULTIBAND_MAX_SAMPLES = pp.MULTIBAND_MAX_SAMPLES
MULTIBAND_WORKSPACE_BYTES = 4 << 30        # multiband_spectra: the workspace it asks for at most (and at least 64 rows)


def multiband_spectra(data_dev, starts, n_samples, frequency_bands, *, sr, buffer_seconds, corners=4,
                      multi_component=False, workspace_bytes=MULTIBAND_WORKSPACE_BYTES):
    """Spectrum.compute_multi_band_spectrum (BPMF/spectrum.py:387-505; method "multiband" of
    compute_moment_magnitude) for the windows of E events, cut from the day in HBM, in one call
    (bpmf_multiband_spectrum_dev, csrc/spectrum.hip): per window the mean and the least-squares line are removed, a
    cosine taper of min(int(0.25 n), int(buffer_seconds sr)) samples is applied on each side, and per frequency band
    the zero-phase Butterworth band-pass of `corners` corners runs over it; the spectrum is max |y| over the window
    less `buffer_seconds` at either end, divided by the bandwidth.  Only these maxima are stored.

    `data_dev`: the (S, C, N) day as a tensor on the GPU, in the units the spectra are wanted in (the instrument
    response is the caller's); `starts` (E,) or (E, S) int64 window starts in samples as in picker_batch;
    `frequency_bands` the reference's dict {name: [lo, hi]} in its order, or a (B, 2) array, in Hz; `sr` in Hz.  The
    noise, P and S windows of the reference's extract_windows are three calls, or one on concatenated starts.
    Returns (spectra, freq, valid) on the day's device and the current stream: `spectra` (E, S, C, B) float64, or
    (E, S, B) with `multi_component` (sqrt of the sum over the components of the squares); `freq` (B,) float32, the
    band centres; `valid` (E, S) bool.  A band with hi >= sr / 2 gives 0, as the reference skips it.  The definition
    is postprocess.multiband_spectrum_host of postprocess.multiband_windows_host; obspy's detrend, taper and filter
    are RESTATED there from their documented behaviour and not yet verified against obspy itself
    (tools/diff_obspy_multiband.py).  A window gives the same bits in any batch and with any `workspace_bytes` (the
    rows go through in slabs of a multiple of 64 that fit it).

    DEPARTURE: a window that is not wholly inside the day gives zeros and valid = False; the reference would filter
    the shorter trace it managed to read.

    Refusals (ValueError, before any device call): data_dev not a GPU tensor or not (S, C, N); n_samples over 16384;
    int(buffer_seconds sr) == 0 or n_samples <= twice that (the reference's data[buf:-buf] is empty there and it
    returns zeros); B outside 1 .. 64; corners outside 1 .. 8; a band with lo <= 0 or lo >= hi; a band with
    (1 - 1e-6) sr / 2 < hi < sr / 2 (obspy silently turns it into a high-pass); rows x B >= 2^31; a workspace too small
    for 64 rows.  Propagation corrections, the network average and Mw* follow in network_average_spectra and
    approximate_moment_magnitudes (source_spectra runs both).  Out of scope: response removal, the `resample` onto
    other target frequencies, and the model fit (fit_average_spectrum: see network_average_spectra)."""
    import ctypes as C
    import torch
    from . import _lib
    S, Cc, N, dev = _day("multiband_spectra", data_dev, "the definition on the host is "
                         "postprocess.multiband_spectrum_host of postprocess.multiband_windows_host")
    n = int(n_samples)
    if not 1 <= n <= MULTIBAND_MAX_SAMPLES:
        raise ValueError(f"multiband_spectra: windows of 1 .. {MULTIBAND_MAX_SAMPLES} samples; got {n}")
    plan = pp.multiband_plan(n, frequency_bands, sr, buffer_seconds, corners)
    st = _window_starts(starts, S)
    E, B = len(st), len(plan["bands"])
    if S * Cc == 0 or N == 0:
        raise ValueError("multiband_spectra: the data are empty")
    rows = st.size * Cc
    if rows * B >= 2**31:
        raise ValueError(f"multiband_spectra: {rows} rows x {B} bands in one call; fewer than 2^31 values fit")
    n_active = int((~plan["skip"]).sum())
    n_bytes = _slab_workspace_bytes(
        lambda r: _lib.lib().bpmf_multiband_workspace_bytes(r, n, n_active), rows, workspace_bytes,
        lambda given, least: f"multiband_spectra: workspace_bytes = {given}; 64 rows of {n} samples and {n_active} "
                             f"active bands take {least}")
    with torch.cuda.device(dev):
        freq = torch.as_tensor(plan["freq"], device=dev)
        spectra = torch.empty((E, S, Cc, B), dtype=torch.float64, device=dev)
        valid = torch.empty((E, S), dtype=torch.uint8, device=dev)
        if E:
            x = data_dev.to(dtype=torch.float32).contiguous()
            d_start = torch.as_tensor(st.reshape(-1), device=dev)
            d_sos = torch.as_tensor(np.ascontiguousarray(plan["sos"]), device=dev)
            ws = torch.empty((n_bytes,), dtype=torch.uint8, device=dev)
            bandwidth = np.ascontiguousarray(plan["bandwidth"], dtype=np.float64)
            skip = np.ascontiguousarray(plan["skip"], dtype=np.uint8)
            _lib.call("bpmf_multiband_spectrum_dev", dev, x, S, Cc, N, st.size, d_start, n, plan["taper"], plan["buffer"],
                      d_sos, B, int(plan["sos"].shape[1]), bandwidth.ctypes.data_as(C.POINTER(C.c_double)),
                      skip.ctypes.data_as(C.POINTER(C.c_uint8)), ws, n_bytes, _lib.STREAM, spectra, valid)
        if multi_component:
            total = torch.zeros((E, S, B), dtype=torch.float64, device=dev)
            for c in range(Cc):                                        # in component order, as the reference adds
                total = total + spectra[:, :, c] * spectra[:, :, c]
            spectra = torch.sqrt(total)
        return spectra, freq, valid.to(torch.bool)


def multiband_snr(signal, noise, noise_valid=None):
    """Spectrum.compute_signal_to_noise_ratio (BPMF/spectrum.py:601-648) on two results of multiband_spectra of equal
    shape (..., B), on their device: 0 where signal and noise are both 0, |signal| / |noise| elsewhere (inf included),
    and 0 where the noise spectrum is missing -- `noise_valid` (...) bool, the `valid` of the noise windows, broadcast
    over the bands (and over the components).  A few elementwise operations on small tensors; the definition is
    postprocess.spectral_snr_host, which it equals exactly.  workflow.spectral_snr is this function under the name
    that fits two results of fft_spectra, (..., F), as well."""
    import torch
    if not isinstance(signal, torch.Tensor) or not isinstance(noise, torch.Tensor) or signal.shape != noise.shape:
        raise ValueError("multiband_snr: signal and noise must be tensors of equal shape (..., B)")
    s, z = signal.abs(), noise.abs()
    keep = ~((s == 0) & (z == 0))
    if noise_valid is not None:
        nv = torch.as_tensor(noise_valid, dtype=torch.bool, device=s.device)
        keep = keep & nv.reshape(tuple(nv.shape) + (1,) * (s.dim() - nv.dim()))
    return torch.where(keep, s / z, torch.zeros_like(s))


spectral_snr = multiband_snr                # the same ratio on two results of fft_spectra


FFT_SPECTRUM_WORKSPACE_BYTES = 1 << 30     # fft_spectra: the workspace it asks for at most (and at least 64 rows)


def target_frequencies(freq_min, freq_max, num_points):
    """Spectrum.set_target_frequencies (BPMF/spectrum.py:920-940): np.logspace(log10(freq_min), log10(freq_max),
    num_points), the `frequencies` of fft_spectra."""
    return np.logspace(np.log10(freq_min), np.log10(freq_max), num_points)


def fft_spectra(data_dev, starts, n_samples, *, sr, frequencies=None, alpha=0.05, taper=None, multi_component=False,
                workspace_bytes=FFT_SPECTRUM_WORKSPACE_BYTES):
    """Spectrum.compute_spectrum and Spectrum.resample (BPMF/spectrum.py:507-599, :851-887; method "regular", the
    default of compute_moment_magnitude) for the windows of E events, cut from the day in HBM, in one call
    (bpmf_fft_spectrum_dev, csrc/fft_spectrum.hip): per window the Tukey taper of `alpha` (or the caller's (n,) `taper`)
    and the Fourier transform times 1 / sr; with `frequencies` the modulus is interpolated linearly onto them as
    np.interp does, and a target at or beyond 0.99 of the last bin's frequency gives 0.  Only the bins next to a
    target are computed: a DFT pruned to them, a float64 matrix product per row with twiddles from an exact table
    (postprocess.dft_twiddles), so n_samples need not be a power of two and no whole spectrum is stored.

    `data_dev`: the (S, C, N) day as a tensor on the GPU, taken as float32, in the units the spectra are wanted in (the
    instrument response is the caller's); `starts` (E,) or (E, S) int64 window starts in samples as in picker_batch;
    `sr` in Hz; `frequencies` (F,) in Hz (target_frequencies), F <= 1024.  The noise, P and S windows of the
    reference's extract_windows are three calls, or one on concatenated starts.
    Returns (spectra, freq, valid) on the day's device and the current stream.  With `frequencies`: `spectra`
    (E, S, C, F) float64, or (E, S, F) with `multi_component` (per bin the root of the sum over the components of
    |X_c|^2, in component order, then interpolated); `freq` (F,) float64 = `frequencies`.  Without: the complex128
    spectrum (E, S, C, n // 2 + 1), or that root (E, S, n // 2 + 1) float64; `freq` = np.fft.rfftfreq(n, 1 / sr).
    `valid` (E, S) bool.  The definition is postprocess.fft_spectrum_host of postprocess.fft_windows_host; every value
    lies within sqrt(2) B / sr + 8 * 2^-53 |value| of it, B = (n + 16) 2^-53 sum_j |x_j taper_j| of the row (of the
    station: the root of its rows' summed B^2), and a window that holds a NaN or an Inf is NaN wherever it is not 0 by the rule
    above.  A window gives the same bits in any batch and with any `workspace_bytes` (the rows go through in slabs of a
    multiple of 64 that fit it).  workflow.spectral_snr is compute_signal_to_noise_ratio on two results.

    DEPARTURE: a window that is not wholly inside the day gives zeros and valid = False; the reference would transform
    the shorter trace it managed to read.

    Refusals (ValueError, before any device call): data_dev not a GPU tensor or not (S, C, N); n_samples outside
    2 .. 16384; sr not positive; alpha outside [0, 1); a taper that is not (n,); no, more than 1024 or non-finite
    frequencies; multi_component with more than 64 components; rows x max(2 bins, F) >= 2^31; a workspace too small for
    64 rows.  Propagation corrections, the network average and Mw* follow in network_average_spectra and
    approximate_moment_magnitudes (source_spectra runs both); `integrate` / `differentiate` are integrate_spectra and
    differentiate_spectra.  Out of scope: response removal, float64 days, a `spectrum_func` callable, and the model
    fit (fit_average_spectrum: see network_average_spectra)."""
    import torch
    from . import _lib
    S, Cc, N, dev = _day("fft_spectra", data_dev, "the definition on the host is postprocess.fft_spectrum_host of "
                                                  "postprocess.fft_windows_host")
    n = int(n_samples)
    plan = pp.fft_spectrum_plan(n, sr, frequencies, alpha, taper)
    st = _window_starts(starts, S)
    E, K_b = len(st), len(plan["bins"])
    F = 0 if frequencies is None else len(plan["frequencies"])
    if S * Cc == 0 or N == 0:
        raise ValueError("fft_spectra: the data are empty")
    multi = bool(multi_component)
    if multi and Cc > 64:
        raise ValueError(f"fft_spectra: multi_component takes at most 64 components; the day has {Cc}")
    rows = st.size * Cc
    if rows * max(2 * K_b, F) >= 2**31:
        raise ValueError(f"fft_spectra: {rows} rows x {max(2 * K_b, F)} values in one call; fewer than 2^31 values fit")
    n_bytes = _slab_workspace_bytes(
        lambda r: _lib.lib().bpmf_fft_spectrum_workspace_size(r, n, K_b, F), rows, workspace_bytes,
        lambda given, least: f"fft_spectra: workspace_bytes = {given}; 64 rows of {n} samples and {K_b} bins take "
                             f"{least}")
    with torch.cuda.device(dev):
        freq = torch.as_tensor(plan["frequencies"] if F else plan["freq"], device=dev)
        lead = (E, S) if multi else (E, S, Cc)
        if F:
            spectra = torch.empty(lead + (F,), dtype=torch.float64, device=dev)
        else:
            spectra = torch.empty(lead + (K_b,), dtype=torch.float64 if multi else torch.complex128, device=dev)
        valid = torch.empty((E, S), dtype=torch.uint8, device=dev)
        if E:
            x = data_dev.to(dtype=torch.float32).contiguous()
            up = {k: torch.as_tensor(np.ascontiguousarray(v), device=dev) for k, v in (
                ("starts", st.reshape(-1)), ("taper", plan["taper"]), ("twiddles", np.array(pp.dft_twiddles(n))),
                ("bins", plan["bins"]))}
            if F:
                up.update({k: torch.as_tensor(np.ascontiguousarray(plan[k]), device=dev)
                           for k in ("pair", "dx", "span", "flags")})
            ws = torch.empty((n_bytes,), dtype=torch.uint8, device=dev)
            _lib.call("bpmf_fft_spectrum_dev", dev, x, S, Cc, N, st.size, up["starts"], n, up["taper"], up["twiddles"],
                      plan["delta"], up["bins"], K_b, up.get("pair"), up.get("dx"), up.get("span"), up.get("flags"), F,
                      int(multi), ws, n_bytes, _lib.STREAM, spectra, valid)
        return spectra, freq, valid.to(torch.bool)


SS_SNR, SS_CORRECT, SS_AVERAGE, SS_MW = 1, 2, 4, 8      # the stages of bpmf_source_spectra_dev


def _source_spectra_shape(name, spectra, other, valid):
    """(E, S, C, F) of two spectra tensors of equal shape (E, S, F) or (E, S, C, F) and their (E, S) `valid`; the
    refusals that need no device."""
    import torch
    for t in (spectra, other):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
            raise ValueError(f"{name}: the spectra must be float64 tensors (as fft_spectra and multiband_spectra "
                             "return them)")
    if spectra.dim() not in (3, 4) or spectra.shape != other.shape:
        raise ValueError(f"{name}: the spectra must be (E, S, F) or (E, S, C, F) and equal in shape; got "
                         f"{tuple(spectra.shape)} and {tuple(other.shape)}")
    E, S, F = int(spectra.shape[0]), int(spectra.shape[1]), int(spectra.shape[-1])
    Cc = 1 if spectra.dim() == 3 else int(spectra.shape[2])
    if tuple(np.shape(valid)) != (E, S):
        raise ValueError(f"{name}: valid must be (E, S) = ({E}, {S}); got {tuple(np.shape(valid))}")
    if not 1 <= S * Cc <= pp.SOURCE_SPECTRA_MAX_CHANNELS:
        raise ValueError(f"{name}: an event takes 1 .. {pp.SOURCE_SPECTRA_MAX_CHANNELS} channels; got S * C = {S * Cc}")
    if not 1 <= F <= pp.SOURCE_SPECTRA_MAX_FREQUENCIES:
        raise ValueError(f"{name}: 1 .. {pp.SOURCE_SPECTRA_MAX_FREQUENCIES} frequencies; got {F}")
    if E * S * Cc * F >= 2**31:
        raise ValueError(f"{name}: {E} events x {S * Cc} channels x {F} frequencies; fewer than 2^31 values fit")
    if not spectra.is_cuda or not other.is_cuda or spectra.device != other.device:
        raise ValueError(f"{name}: the spectra must be tensors on one GPU (there is no CPU path; the definitions on "
                         "the host are postprocess.source_spectra_host and approximate_moment_magnitude_host)")
    return E, S, Cc, F


def _per_station(name, what, value, shape, dev, dtype):
    import torch
    if tuple(np.shape(value)) != shape:
        raise ValueError(f"{name}: {what} must be {shape}; got {tuple(np.shape(value))}")
    value = value if isinstance(value, torch.Tensor) else np.array(value)      # (a copy: the array may be read-only)
    return torch.as_tensor(value).to(device=dev, dtype=dtype).contiguous()


def network_average_spectra(signal, noise, *, phase, valid, noise_valid=None, dist_km, tt_p_sec, tt_s_sec,
                            location_err_km, frequencies, medium, q_phase_prefactor=None, attenuation="reference",
                            radiation=None, snr_threshold, average_log=True, min_num_valid_channels_per_freq_bin=0,
                            max_relative_distance_err_pct=25.0, reduce="mean"):
    """What compute_moment_magnitude does between the spectra and the model fit (BPMF/spectrum.py:1801-1867) for one
    phase ("p" or "s") of E events, in one call on the device (bpmf_source_spectra_dev, csrc/source_spectra.hip):
    compute_signal_to_noise_ratio, correct_geometrical_spreading, correct_attenuation and
    compute_network_average_spectrum.

    `signal`, `noise`: (E, S, F) or (E, S, C, F) float64 tensors on the GPU, as fft_spectra / multiband_spectra return
    them for the phase's and the noise windows, on the `frequencies` (F,) given (a resample of multi-band spectra onto
    other targets is the caller's); `valid`, `noise_valid` (E, S) bool: their `valid` (noise_valid None: all there).
    `dist_km`, `tt_p_sec`, `tt_s_sec` (E, S): source-receiver distances and travel times; `location_err_km` (E,):
    sqrt(hmax_unc^2 + vmax_unc^2); `medium`: the reference's medium_properties (postprocess.MEDIUM_KEYS);
    `radiation`: the phase's radiation coefficient (None: sqrt(4/15) for P, sqrt(2/5) for S).
    attenuation="reference" keeps what the reference does (postprocess.attenuation_plan): BOTH phases are corrected
    with the S travel time, the P factor with Q * prefactor["s"] and the S factor with Q * prefactor["p"];
    attenuation="physical" pairs tt_p with Q_p and tt_s with Q_s.

    Returns a dict of tensors on the inputs' device and the current stream: `corrected`, `snr` (shaped as `signal`),
    `average`, `std` (E, F) float64 (NaN where `mask`), `mask` (E, F) bool, `num_valid` (E, F) int32 and `used` (E, S)
    bool.  The (E, F) averages are exactly what Spectrum.fit_average_spectrum takes.  That fit (SciPy's curve_fit: TRF
    with a 2-point Jacobian on parameters of scale 1e11 .. 1e15 and 1 .. 30 with x_scale = 1) is not offered: its
    answer is a property of SciPy's termination rules, not a definition.  The definition is
    postprocess.source_spectra_host; bounds in DESIGN.md section 4.  An event gives the same bits alone and in any batch.
    Since then the fit is offered as the exact least-squares minimum: fit_source_spectra; and resample_spectra puts
    multi-band spectra onto other targets.

    Refusals (ValueError, before any device call): spectra that are no float64 tensors of equal shape (E, S, F) or
    (E, S, C, F) on one GPU; S * C above 256; F above 1024; E S C F >= 2^31; a per-station table that is not (E, S);
    a phase, reduce or attenuation that is not one of the two; frequencies that are not (F,) finite numbers."""
    import torch
    from . import _lib
    name = "network_average_spectra"
    if phase not in ("p", "s"):
        raise ValueError(f"{name}: phase must be 'p' or 's'; got {phase!r}")
    if reduce not in ("mean", "median"):
        raise ValueError(f"{name}: reduce must be 'mean' or 'median'; got {reduce!r}")
    k = ("p", "s").index(phase)
    f = np.array(frequencies.detach().cpu().numpy() if isinstance(frequencies, torch.Tensor) else frequencies,
                 dtype=np.float64)                                     # (a copy: it is uploaded, and may be read-only)
    which, q_rows = pp.attenuation_plan(f, medium, q_phase_prefactor, attenuation)
    if isinstance(signal, torch.Tensor) and signal.dim() in (3, 4) and signal.shape[-1] != len(f):
        raise ValueError(f"{name}: the spectra hold {signal.shape[-1]} frequencies, `frequencies` {len(f)}")
    E, S, Cc, F = _source_spectra_shape(name, signal, noise, valid)
    constant = float(pp.geometry_constants(medium)[k])
    radiation = float((pp.RADIATION_P, pp.RADIATION_S)[k] if radiation is None else radiation)
    dev = signal.device
    with torch.cuda.device(dev):
        tab = {"valid": _per_station(name, "valid", valid, (E, S), dev, torch.uint8),
               "noise_valid": _per_station(name, "noise_valid", np.ones((E, S), bool) if noise_valid is None
                                           else noise_valid, (E, S), dev, torch.uint8),
               "dist": _per_station(name, "dist_km", dist_km, (E, S), dev, torch.float64),
               "tt": _per_station(name, "tt_p_sec / tt_s_sec", tt_p_sec if which[k] == "p" else tt_s_sec, (E, S), dev,
                                  torch.float64),
               "err": _per_station(name, "location_err_km", location_err_km, (E,), dev, torch.float64),
               "f": torch.as_tensor(f, device=dev), "q": torch.as_tensor(np.ascontiguousarray(q_rows[k]), device=dev)}
        x, z = signal.contiguous(), noise.contiguous()
        out = {"corrected": torch.empty_like(x), "snr": torch.empty_like(x),
               "average": torch.empty((E, F), dtype=torch.float64, device=dev),
               "mask": torch.empty((E, F), dtype=torch.uint8, device=dev),
               "std": torch.empty((E, F), dtype=torch.float64, device=dev),
               "num_valid": torch.empty((E, F), dtype=torch.int32, device=dev),
               "used": torch.empty((E, S), dtype=torch.uint8, device=dev)}
        if E:
            p = {**tab, **out}
            _lib.call("bpmf_source_spectra_dev", dev, x, z, p["valid"], p["noise_valid"], p["dist"], None, p["tt"],
                      p["err"], p["f"], p["q"], E, S, Cc, F, SS_SNR | SS_CORRECT | SS_AVERAGE, constant, radiation,
                      float(snr_threshold), float(max_relative_distance_err_pct),
                      int(min_num_valid_channels_per_freq_bin), int(bool(average_log)), int(reduce == "median"), 1, 0,
                      0.0, 0.0, 0, _lib.STREAM, p["corrected"], p["snr"], p["average"], p["mask"], p["std"],
                      p["num_valid"], p["used"], None, None, None, None, None)
        out["mask"], out["used"] = out["mask"].to(torch.bool), out["used"].to(torch.bool)
        return out


def approximate_moment_magnitudes(corrected, snr, *, valid, frequencies, epicentral_dist_km, snr_threshold=10.0,
                                  num_averaging_bands=1, low_snr_freq_min_hz=2.0,
                                  magnitude_log_moment_scaling=2.0 / 3.0, weight_max=3.0, max_num_bad_measurements=6):
    """approximate_moment_magnitude (BPMF/spectrum.py:1341-1496, with _snr_based_weights :1290-1338) of one phase of E
    events in one call on the device (bpmf_source_spectra_dev, stage 8): `corrected` and `snr` as
    network_average_spectra returns them, `valid` (E, S) bool, `frequencies` (F,) ascending, `epicentral_dist_km`
    (E, S).  The reference's dtypes are kept: the measurements' SNR and the weights are float32, the weights' sum a
    float32 sum in NumPy's order.  The reference indexes the distances by spectrum id and so runs only with
    multi_component_spectrum=True; here a channel of (E, S, C, F) spectra takes the distance of its station.
    Returns a dict of tensors: `Mw_star`, `log10_M0` (E,) float64 (NaN for an event without a positive weight),
    `measured_disp` (E, S * C) float64 (NaN for a station that is not valid), `weights`, `measurement_snr` (E, S * C)
    float32.  The definition is postprocess.approximate_moment_magnitude_host; bounds in DESIGN.md section 4.
    Refusals (ValueError, before any device call): as network_average_spectra; num_averaging_bands outside 1 .. 8;
    frequencies that do not ascend; max_num_bad_measurements < 0."""
    import torch
    from . import _lib
    name = "approximate_moment_magnitudes"
    f = np.ascontiguousarray(frequencies.detach().cpu().numpy() if isinstance(frequencies, torch.Tensor)
                             else frequencies, dtype=np.float64)
    if f.ndim != 1 or not np.isfinite(f).all() or np.any(np.diff(f) <= 0):
        raise ValueError(f"{name}: frequencies must be (F,) finite, ascending numbers")
    nab = int(num_averaging_bands)
    if not 1 <= nab <= pp.SOURCE_SPECTRA_MAX_AVERAGING_BANDS:
        raise ValueError(f"{name}: num_averaging_bands must be 1 .. {pp.SOURCE_SPECTRA_MAX_AVERAGING_BANDS}; got {nab}")
    if int(max_num_bad_measurements) < 0:
        raise ValueError(f"{name}: max_num_bad_measurements must not be negative")
    if isinstance(corrected, torch.Tensor) and corrected.dim() in (3, 4) and corrected.shape[-1] != len(f):
        raise ValueError(f"{name}: the spectra hold {corrected.shape[-1]} frequencies, `frequencies` {len(f)}")
    E, S, Cc, F = _source_spectra_shape(name, corrected, snr, valid)
    first_high = int(np.searchsorted(f, low_snr_freq_min_hz, side="right"))        # the bands with f > the minimum
    dev = corrected.device
    with torch.cuda.device(dev):
        v = _per_station(name, "valid", valid, (E, S), dev, torch.uint8)
        epi = _per_station(name, "epicentral_dist_km", epicentral_dist_km, (E, S), dev, torch.float64)
        x, r = corrected.contiguous(), snr.contiguous()
        out = {"Mw_star": torch.empty((E,), dtype=torch.float64, device=dev),
               "log10_M0": torch.empty((E,), dtype=torch.float64, device=dev),
               "measured_disp": torch.empty((E, S * Cc), dtype=torch.float64, device=dev),
               "weights": torch.empty((E, S * Cc), dtype=torch.float32, device=dev),
               "measurement_snr": torch.empty((E, S * Cc), dtype=torch.float32, device=dev)}
        if E:
            _lib.call("bpmf_source_spectra_dev", dev, None, None, v, None, None, epi, None, None, None, None, E, S, Cc,
                      F, SS_MW, 0.0, 1.0, float(snr_threshold), 0.0, 0, 0, 0, nab, first_high,
                      float(magnitude_log_moment_scaling), float(weight_max), int(max_num_bad_measurements),
                      _lib.STREAM, x, r, None, None, None, None, None, out["Mw_star"], out["log10_M0"],
                      out["measured_disp"], out["weights"], out["measurement_snr"])
        return out


def source_spectra(*, p=None, s=None, noise, valid_p=None, valid_s=None, noise_valid=None, dist_km,
                   epicentral_dist_km, tt_p_sec, tt_s_sec, location_err_km, frequencies, medium, snr_threshold,
                   q_phase_prefactor=None, attenuation="reference", average_log=True,
                   min_num_valid_channels_per_freq_bin=0, max_relative_distance_err_pct=25.0, reduce="mean",
                   num_averaging_bands=1, low_snr_freq_min_hz=2.0, magnitude_log_moment_scaling=2.0 / 3.0,
                   weight_max=3.0, max_num_bad_measurements=6, fit=None, fit_weighted=True, fit_on="average",
                   min_fraction_valid_points=0.5, min_fraction_valid_points_below_fc=0.1):
    """network_average_spectra, then approximate_moment_magnitudes, for each phase given (`p`, `s`: the phase's
    spectra; `valid_p`, `valid_s`: their `valid`): a day's events go from the spectra in HBM to (E, F) network-average
    source spectra and a per-event Mw* in two calls per phase.  Returns {"p": {...}, "s": {...}} for the phases given,
    each the two functions' dicts in one.  The phases are NOT combined: the reference's combined Mw* is, through a
    misplaced `if` (BPMF/spectrum.py:1879-1880), the last phase's value alone; the caller averages as they see fit.
    With fit="brune" or "boatwright" each phase's dict gains the keys of fit_source_spectra (weighted=fit_weighted and
    the two fractions), run on the returned `average` or, with fit_on="integrated", on integrate_spectra of it;
    moment_magnitudes combines the two phases.  fit=None (the default) adds nothing."""
    if fit is not None and fit not in pp.FIT_MODELS:
        raise ValueError(f"source_spectra: fit must be None or one of {sorted(pp.FIT_MODELS)}; got {fit!r}")
    if fit_on not in ("average", "integrated"):
        raise ValueError(f"source_spectra: fit_on must be 'average' or 'integrated'; got {fit_on!r}")
    given = [(ph, x, v) for ph, x, v in (("p", p, valid_p), ("s", s, valid_s)) if x is not None]
    if not given:
        raise ValueError("source_spectra: give the spectra of at least one phase (p=, s=)")
    out = {}
    for ph, x, v in given:
        if v is None:
            raise ValueError(f"source_spectra: valid_{ph} is needed beside {ph}=")
        out[ph] = network_average_spectra(
            x, noise, phase=ph, valid=v, noise_valid=noise_valid, dist_km=dist_km, tt_p_sec=tt_p_sec,
            tt_s_sec=tt_s_sec, location_err_km=location_err_km, frequencies=frequencies, medium=medium,
            q_phase_prefactor=q_phase_prefactor, attenuation=attenuation, snr_threshold=snr_threshold,
            average_log=average_log, min_num_valid_channels_per_freq_bin=min_num_valid_channels_per_freq_bin,
            max_relative_distance_err_pct=max_relative_distance_err_pct, reduce=reduce)
        out[ph].update(approximate_moment_magnitudes(
            out[ph]["corrected"], out[ph]["snr"], valid=v, frequencies=frequencies,
            epicentral_dist_km=epicentral_dist_km, snr_threshold=snr_threshold,
            num_averaging_bands=num_averaging_bands, low_snr_freq_min_hz=low_snr_freq_min_hz,
            magnitude_log_moment_scaling=magnitude_log_moment_scaling, weight_max=weight_max,
            max_num_bad_measurements=max_num_bad_measurements))
        if fit is not None:
            spectrum = out[ph]["average"]
            if fit_on == "integrated":
                spectrum = integrate_spectra(spectrum, frequencies)
            out[ph].update(fit_source_spectra(
                spectrum, out[ph]["mask"], out[ph]["num_valid"], frequencies=frequencies, phase=ph, model=fit,
                weighted=fit_weighted, min_fraction_valid_points=min_fraction_valid_points,
                min_fraction_valid_points_below_fc=min_fraction_valid_points_below_fc))
    return out


def fit_source_spectra(average, mask, num_valid, *, frequencies, phase, model="brune", weighted=False,
                       min_fraction_valid_points=0.5, min_fraction_valid_points_below_fc=0.1):
    """Spectrum.fit_average_spectrum (BPMF/spectrum.py:729-849, log=True), the below-fc gate and the stress drop for
    one phase of E events in one call on the device (bpmf_fit_spectra_dev, csrc/spectral_fit.hip): `average` (E, F)
    float64, `mask` (E, F) bool and `num_valid` (E, F) int32 as network_average_spectra returns them (or
    integrate_spectra of the average), `frequencies` (F,).  The fit is defined as the exact weighted least-squares
    minimum, found by profiling over ln fc with log10 Omega_0 in closed form -- not as the point where SciPy's
    curve_fit stops (its cost is never below this one's); the definition, its bounds, its covariance and its
    departures from the reference are postprocess.fit_source_spectra_host's, DESIGN.md section 4.

    Returns a dict of (E,) tensors on the inputs' device and the current stream: `M0`, `fc`, `Mw`, `M0_err`, `fc_err`,
    `cost`, `stress_drop_pa` float64 (NaN where nothing was fitted), `n_valid` int32, `success`, `at_bound` bool and
    `reason` uint8 (postprocess.FIT_REASONS).  An event gives the same bits alone and in any batch.

    Refusals (ValueError, before any device call): average, mask, num_valid that are not (E, F) tensors of float64,
    bool (or uint8) and int32 on one GPU; F outside 1 .. 1024; E F >= 2^31; a model that is not "brune" or
    "boatwright"; a phase that is not "p" or "s"; frequencies that are not (F,) finite, positive and ascending."""
    import torch
    from . import _lib
    name = "fit_source_spectra"
    if model not in pp.FIT_MODELS:
        raise ValueError(f"{name}: model must be one of {sorted(pp.FIT_MODELS)}; got {model!r}")
    if phase not in ("p", "s"):
        raise ValueError(f"{name}: phase must be 'p' or 's'; got {phase!r}")
    f = np.array(frequencies.detach().cpu().numpy() if isinstance(frequencies, torch.Tensor) else frequencies,
                 dtype=np.float64)
    if f.ndim != 1 or not np.isfinite(f).all() or np.any(f <= 0) or np.any(np.diff(f) <= 0):
        raise ValueError(f"{name}: frequencies must be (F,) finite, positive, ascending numbers")
    for what, t, dtypes in (("average", average, (torch.float64,)), ("mask", mask, (torch.bool, torch.uint8)),
                            ("num_valid", num_valid, (torch.int32,))):
        if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or t.dim() != 2:
            raise ValueError(f"{name}: {what} must be an (E, F) tensor of {' or '.join(str(d) for d in dtypes)}")
    if average.shape != mask.shape or average.shape != num_valid.shape or average.shape[1] != len(f):
        raise ValueError(f"{name}: average, mask and num_valid must be (E, F) with F = {len(f)} frequencies; got "
                         f"{tuple(average.shape)}, {tuple(mask.shape)}, {tuple(num_valid.shape)}")
    E, F = int(average.shape[0]), int(average.shape[1])
    if not 1 <= F <= pp.SOURCE_SPECTRA_MAX_FREQUENCIES:
        raise ValueError(f"{name}: 1 .. {pp.SOURCE_SPECTRA_MAX_FREQUENCIES} frequencies; got {F}")
    if E * F >= 2**31:
        raise ValueError(f"{name}: {E} events x {F} frequencies; fewer than 2^31 values fit")
    if not average.is_cuda or mask.device != average.device or num_valid.device != average.device:
        raise ValueError(f"{name}: average, mask and num_valid must be tensors on one GPU (there is no CPU path; the "
                         "definition on the host is postprocess.fit_source_spectra_host)")
    dev = average.device
    with torch.cuda.device(dev):
        out = {k: torch.empty((E,), dtype=torch.float64, device=dev) for k in pp.FIT_KEYS}
        out["n_valid"] = torch.empty((E,), dtype=torch.int32, device=dev)
        flags = {k: torch.empty((E,), dtype=torch.uint8, device=dev) for k in ("success", "at_bound", "reason")}
        if E:
            _lib.call("bpmf_fit_spectra_dev", dev, average.contiguous(), mask.to(torch.uint8).contiguous(),
                      num_valid.contiguous(), torch.as_tensor(f, device=dev), E, F, ("brune", "boatwright").index(model),
                      ("p", "s").index(phase), int(bool(weighted)), float(min_fraction_valid_points),
                      float(min_fraction_valid_points_below_fc), _lib.STREAM, *(out[k] for k in pp.FIT_KEYS),
                      out["n_valid"], flags["success"], flags["at_bound"], flags["reason"])
        out.update(success=flags["success"].to(torch.bool), at_bound=flags["at_bound"].to(torch.bool),
                   reason=flags["reason"])
        return out


def moment_magnitudes(fit_p=None, fit_s=None, *, max_rel_m0_err_pct=33.0, max_rel_fc_err_pct=33.0):
    """The acceptance tests and the P-S average of compute_moment_magnitude (BPMF/spectrum.py:1907-1946, :1965-1990) on
    the dicts of fit_source_spectra, as torch operations on their (E,) tensors: a phase is accepted where its fit
    succeeded and not (100 M0_err / M0 > max_rel_m0_err_pct or fc < 0 or 100 fc_err / fc > max_rel_fc_err_pct); `Mw`
    and `Mw_err` (of 2 / 3 * M0_err / M0) are the accepted phases' sums, P first, divided by their number, NaN where no
    phase was accepted.  The stress-drop gate that the reference overrides to True stays overridden.  Returns
    {"Mw", "Mw_err": (E,) float64, "accepted": {phase: (E,) bool}}; the definition is
    postprocess.moment_magnitudes_host."""
    import torch
    given = [(ph, fit) for ph, fit in (("p", fit_p), ("s", fit_s)) if fit is not None]
    if not given:
        raise ValueError("moment_magnitudes: give the fit of at least one phase (fit_p=, fit_s=)")
    like = given[0][1]["M0"]
    total, total_err, norm, accepted = torch.zeros_like(like), torch.zeros_like(like), torch.zeros_like(like), {}
    zero = torch.zeros_like(like)
    for ph, fit in given:
        rel_m0 = 100.0 * fit["M0_err"] / fit["M0"]
        rel_fc = 100.0 * fit["fc_err"] / fit["fc"]
        ok = fit["success"] & ~((rel_m0 > max_rel_m0_err_pct) | (fit["fc"] < 0.0) | (rel_fc > max_rel_fc_err_pct))
        accepted[ph] = ok
        total = total + torch.where(ok, fit["Mw"], zero)
        total_err = total_err + torch.where(ok, 2.0 / 3.0 * fit["M0_err"] / fit["M0"], zero)
        norm = norm + ok.to(like.dtype)
    nan = torch.full_like(like, float("nan"))
    return {"Mw": torch.where(norm > 0, total / norm, nan), "Mw_err": torch.where(norm > 0, total_err / norm, nan),
            "accepted": accepted}


def resample_spectra(spectra, frequencies_in, frequencies_out):
    """Spectrum.resample (BPMF/spectrum.py:851-887) for multi-band spectra on the device: (..., B) spectra on the bands'
    `frequencies_in` (B,) onto `frequencies_out` (T,), by np.interp's formula with one rounded operation each --
    ((fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j])) (x - xp[j]) + fp[j] of |spectra|, fp[j] itself on a band's frequency,
    the end values outside the bands -- and +0 at and beyond 0.99 max(frequencies_in).  Returns (..., T) on the
    spectra's device, bit for bit what postprocess.resample_spectra_host gives (no product is fused with a sum: each
    is a torch operation of its own).  ValueError for spectra that are no floating-point tensor on the GPU with B as
    their last axis, and for frequencies that postprocess.resample_plan refuses."""
    import torch
    name = "resample_spectra"
    f_in = _spectra_and_frequencies(name, spectra, frequencies_in)
    plan = pp.resample_plan(f_in.detach().cpu().numpy(), frequencies_out.detach().cpu().numpy()
                            if isinstance(frequencies_out, torch.Tensor) else frequencies_out)
    dev = spectra.device
    t = {k: torch.as_tensor(np.ascontiguousarray(v), device=dev) for k, v in plan.items()}
    dx, span = t["dx"].to(spectra.dtype), t["span"].to(spectra.dtype)
    fp = spectra.abs()
    lo, hi = fp[..., t["pair"]], fp[..., t["pair"] + 1]
    slope = (hi - lo) / span
    out = slope * dx + lo
    # np.interp's own second thoughts on a NaN: from the pair's other end, then equal ends
    out = torch.where(out.isnan(), slope * (dx - span) + hi, out)
    out = torch.where(out.isnan() & (lo == hi), lo, out)
    out = torch.where(t["on"], lo, out)
    out = torch.where(t["below"], fp[..., :1], out)
    out = torch.where(t["above"], fp[..., -1:], out)
    return torch.where(t["outside"], torch.zeros_like(out), out)


def _spectra_and_frequencies(name, spectra, frequencies):
    import torch
    if not isinstance(spectra, torch.Tensor) or not spectra.is_cuda or not spectra.is_floating_point():
        raise ValueError(f"{name}: spectra must be a floating-point tensor on the GPU")
    f = torch.as_tensor(frequencies if isinstance(frequencies, torch.Tensor) else np.array(frequencies))
    f = f.to(device=spectra.device, dtype=spectra.dtype)
    if f.dim() != 1 or spectra.dim() < 1 or spectra.shape[-1] != f.shape[0]:
        raise ValueError(f"{name}: frequencies must be (F,) with F the spectra's last axis")
    return f


def integrate_spectra(spectra, frequencies):
    """Spectrum.integrate (BPMF/spectrum.py:650-687): the spectra (..., F), single ones or network averages, divided
    by their frequencies -- one rounded division each, on the spectra's device."""
    return spectra / _spectra_and_frequencies("integrate_spectra", spectra, frequencies)


def differentiate_spectra(spectra, frequencies):
    """Spectrum.differentiate (BPMF/spectrum.py:689-727): the spectra (..., F) times their frequencies."""
    return spectra * _spectra_and_frequencies("differentiate_spectra", spectra, frequencies)


def _peak_amplitude_window(sr, offset_win_peak_amp_sec, duration_win_peak_amp_sec):
    """(offset, duration) in samples, as MatchedFilter.set_data converts them (BPMF/similarity_search.py:175-180)."""
    return (int(pp.sec_to_samp(offset_win_peak_amp_sec, sr)), int(pp.sec_to_samp(duration_win_peak_amp_sec, sr)))


def _split_by_row(rows, values, n_rows):
    """(D, ...) values of detections sorted by row -> {row: values of that row} for every row of range(n_rows)."""
    bounds = np.searchsorted(rows, np.arange(n_rows + 1))
    return {t: values[bounds[t]:bounds[t + 1]] for t in range(n_rows)}


def detection_aux_data(detections_with_values, amplitudes, n_dev, tids=None):
    """The ``aux_data`` dict the reference attaches to every detection (BPMF/similarity_search.py:715-722), per
    template row: {row: [dict, ...]} in the order of the detections.  `detections_with_values`: {row: (cc indices,
    cc float32, threshold float32)} (cc_detections(with_values=True), sharded_matched_filter_detections);
    `amplitudes`: {row: (n_row, S, C)} (matched_filter_detections(extract_peak_amplitudes=True)) or None -- the
    reference then stores no "peak_amplitudes"; `n_dev`: cfg.N_DEV_MF_THRESHOLD; `tids`: the template ids of the rows
    (default: the row itself).  float32 arithmetic: n_threshold = cc / threshold, n_dev = n_threshold * n_dev."""
    out = {}
    for t, (idx, val, thr) in detections_with_values.items():
        val = np.asarray(val, dtype=np.float32)
        thr = np.asarray(thr, dtype=np.float32)
        events = []
        for i in range(len(idx)):
            aux = {"cc": val[i], "n_threshold": val[i] / thr[i]}
            aux["n_dev"] = aux["n_threshold"] * np.float32(n_dev)
            aux["tid"] = t if tids is None else tids[t]
            if amplitudes is not None:
                aux["peak_amplitudes"] = amplitudes[t][i]
            events.append(aux)
        out[t] = events
    return out


def matched_filter_detections(templates, moveouts, weights, data, *, step=1, sr,
                              threshold_window_dur, minimum_interevent_time, n_dev=8.0,
                              overlap=0.25, max_cc_threshold=0.80, white_noise=None, device=None,
                              remove_edges=True, data_buffer_sec=None, data_duration_sec=None,
                              sanity_check=True, max_kurto=100.0, threshold_type="rms",
                              anomalous_cdf_at_mean_plus_1sig=0.0, window_for_validation_Tmax=100.0, min_freq_hz=None,
                              extract_peak_amplitudes=False, offset_win_peak_amp_sec=1.0,
                              duration_win_peak_amp_sec=3.0, moveouts_peak_amp=None, data_norm=None,
                              normalize="short"):
    """Matched-filter search of one day: returns ({template: cc indices}, cc device tensor).

    `normalize`: "short" (the mode the reference uses) or "full" -- the window mean removed, for days whose windows are
    not zero-mean (matched_filter_full); everything behind the CC matrix is the same.

    `extract_peak_amplitudes` (the reference's default, BPMF/similarity_search.py:733, 695-714; off here, so that
    the return value stays the pair): returns (detections, cc, amplitudes) with amplitudes = {row: (n_row, S, C)
    float32} in the order of detections[row] -- per channel the maximum of the day in the `duration_win_peak_amp_sec`
    window that starts `offset_win_peak_amp_sec` before the arrival, times `data_norm` (S, C) (normalize_data(...,
    return_norm=True); None: the amplitudes of the day as given).  `moveouts_peak_amp` (T, S, C): the moveouts of the
    phases of `phase_on_comp_peak_amp` in samples (default: `moveouts`).  Gathered on the device from the day the
    matched filter holds there (peak_amplitudes): no second upload.

    `remove_edges` (the reference's default, BPMF/similarity_search.py:274-285) drops detections
    inside the `data_buffer_sec` margins the day was loaded with (`cfg.DATA_BUFFER_SEC`) and past
    `data_duration_sec + data_buffer_sec`; it needs `data_buffer_sec` (pass remove_edges=False for a
    day loaded without margins).  The optional anomalous-CDF validation of :253-272
    (`anomalous_cdf_at_mean_plus_1sig` > 0 with `min_freq_hz`; off by default like the reference's class default)
    runs on the device too, see cc_detections.  `sanity_check` (the reference's default, :633-642): a
    template whose CC series has an excess kurtosis above `max_kurto` -- most of the day missing --
    yields no detection (the reference zeroes its CCs before the peak selection); `threshold_type`:
    the RMS threshold of libc.c (default) or the MAD threshold of similarity_search.py:1079-1113; the kurtosis is
    scipy.stats.kurtosis of the float32 row, evaluated on the device in SciPy's own float32 order.
    `remove_edges=True` without `data_buffer_sec` raises: the reference always trims
    cfg.DATA_BUFFER_SEC, there is no silent default here."""
    if remove_edges and data_buffer_sec is None:
        raise ValueError("remove_edges=True needs data_buffer_sec (the reference trims cfg.DATA_BUFFER_SEC); "
                         "pass remove_edges=False for a day without margins")
    weights = np.asarray(weights, dtype=np.float32)
    mf = MatchedFilterGPU(device=device)
    mf.set_data(data)
    cc = mf.run(templates, moveouts, weights, step, normalize=normalize)
    out = cc_detections(cc, moveouts, weights, step=step, sr=sr, threshold_window_dur=threshold_window_dur,
                        minimum_interevent_time=minimum_interevent_time, n_dev=n_dev, overlap=overlap,
                        max_cc_threshold=max_cc_threshold, white_noise=white_noise, device=device,
                        remove_edges=remove_edges, data_buffer_sec=data_buffer_sec,
                        data_duration_sec=data_duration_sec, sanity_check=sanity_check, max_kurto=max_kurto,
                        threshold_type=threshold_type, anomalous_cdf_at_mean_plus_1sig=anomalous_cdf_at_mean_plus_1sig,
                        window_for_validation_Tmax=window_for_validation_Tmax, min_freq_hz=min_freq_hz)
    if not extract_peak_amplitudes:
        return out, cc
    offset, duration = _peak_amplitude_window(sr, offset_win_peak_amp_sec, duration_win_peak_amp_sec)
    n_t = weights.shape[0]
    rows = np.concatenate([np.full(len(out[t]), t, dtype=np.int32) for t in range(n_t)])
    samples = np.concatenate([np.asarray(out[t], dtype=np.int64) * step for t in range(n_t)])
    amp = peak_amplitudes(mf.data, rows, samples, moveouts if moveouts_peak_amp is None else moveouts_peak_amp,
                          offset=offset, duration=duration, data_norm=data_norm)
    return out, cc, _split_by_row(rows, amp, n_t)


def cc_detections(cc, moveouts, weights, *, step=1, sr, threshold_window_dur, minimum_interevent_time,
                  n_dev=8.0, overlap=0.25, max_cc_threshold=0.80, white_noise=None, device=None,
                  remove_edges=True, data_buffer_sec=None, data_duration_sec=None, sanity_check=True,
                  max_kurto=100.0, threshold_type="rms", with_values=False, timings=None,
                  anomalous_cdf_at_mean_plus_1sig=0.0, window_for_validation_Tmax=100.0, min_freq_hz=None):
    """The detection stage of matched_filter_detections on a (T, n_corr) CC matrix that already lies in
    HBM (``MatchedFilter.find_detections``, BPMF/similarity_search.py:548-666): NaN scrub, threshold and
    candidates on the device, the reference's pair-wise merge, kurtosis sanity check, edge removal.
    `moveouts` / `weights` are those of the rows of `cc`.  Returns {row: cc indices}; with
    `with_values` {row: (cc indices, cc values float32, threshold values float32)}.  `timings`: a dict
    that receives "threshold_ms" / "candidates_ms" / "merge_ms" / "candidates" (the device is synchronised
    around the stages only when it is given).

    `anomalous_cdf_at_mean_plus_1sig` > 0 (the class default of the reference is 0.0 = off, similarity_search.py:40;
    its select_cc_indexes defaults to 0.50): the validation of :253-272 between the merge and the edge removal --
    around every merged detection, two adjacent windows of the CC row (together int(window_for_validation_Tmax /
    min_freq_hz) samples, the reference's own unit) must each hold at least that fraction of samples below
    threshold / n_dev (x 1.48 under the MAD threshold), or the threshold is deemed to have failed there and the
    detection is dropped.  The counts are taken on the device (bpmf_count_below_dev: one workgroup per detection),
    the CC rows stay in HBM; needs `min_freq_hz` (cfg.MIN_FREQ_HZ)."""
    import time
    if remove_edges and data_buffer_sec is None:
        raise ValueError("remove_edges=True needs data_buffer_sec (the reference trims cfg.DATA_BUFFER_SEC); "
                         "pass remove_edges=False for a day without margins")
    weights = np.asarray(weights, dtype=np.float32)
    if device is None and hasattr(cc, "device"):
        device = cc.device.index
    cc.nan_to_num_(nan=0.0)                                    # similarity_search.py:540
    th = ThresholdGPU(device=device)

    def clock():
        if timings is None:
            return 0.0
        import torch
        torch.cuda.synchronize(cc.device)
        return time.perf_counter()

    t_0 = clock()
    window = int(pp.sec_to_samp(threshold_window_dur, sr))
    threshold_type = threshold_type.lower()
    if threshold_type == "rms":
        thr_win, _ = th.time_dependent_threshold(cc, window, n_dev, overlap=overlap,
                                                 white_noise=white_noise)
    elif threshold_type == "mad":                                               # :1079-1113
        # The reference fills the zeros of a series with white_noise[:n_zeros] and draws one value per
        # sample; a shorter array (the 500 values the RMS variant cycles through) is repeated up to
        # the series length here -- the reference itself would fail to broadcast it.
        if white_noise is not None and len(white_noise) < cc.shape[-1]:
            white_noise = np.resize(np.asarray(white_noise, dtype=np.float32), cc.shape[-1])
        thr_win, _ = th.time_dependent_threshold_mad(cc, window, n_dev, overlap=overlap,
                                                     white_noise=white_noise, expand=False)
    else:
        raise ValueError("threshold_type must be 'rms' or 'mad'")
    t_1 = clock()
    cap = max_cc_threshold * weights.reshape(weights.shape[0], -1).sum(axis=1)   # :629
    cand = th.extract_candidates(cc, thr_win, window, overlap=overlap, row_cap=cap, kind=threshold_type)
    t_2 = clock()
    min_iet = int(pp.sec_to_samp(minimum_interevent_time, sr))
    mv = np.asarray(moveouts)
    rejected = row_excess_kurtosis(cc) > max_kurto if sanity_check else np.zeros(weights.shape[0], bool)
    out = {}
    # (the candidates come sorted by row, then index: the rows are slices of four plain arrays, not 500 masks over
    # all records and field views of each; the search windows of all templates in one go)
    n_t = weights.shape[0]
    bounds = np.searchsorted(cand["row"], np.arange(n_t + 1))
    c_index = np.ascontiguousarray(cand["index"])
    c_cc = np.ascontiguousarray(cand["cc"])
    c_thr = np.ascontiguousarray(cand["threshold"])
    wins = search_windows(mv.reshape(n_t, mv.shape[1], -1), min_iet, step)
    lo_edge = pp.sec_to_samp(data_buffer_sec, sr) if remove_edges else None
    hi_edge = pp.sec_to_samp(data_duration_sec + data_buffer_sec, sr) if remove_edges and data_duration_sec is not None else None
    empty = (np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros(0, np.float32)) if with_values \
        else np.zeros(0, dtype=np.int64)
    merged = {}
    for t in range(n_t):
        if not rejected[t]:
            b0, b1 = bounds[t], bounds[t + 1]
            merged[t] = merge_candidates(c_index[b0:b1], c_cc[b0:b1], wins[t])
    if anomalous_cdf_at_mean_plus_1sig > 0.0:
        if min_freq_hz is None:
            raise ValueError("anomalous_cdf_at_mean_plus_1sig > 0 needs min_freq_hz (the reference's cfg.MIN_FREQ_HZ)")
        merged = validate_detections(cc, merged, bounds, c_index, c_thr, n_dev=n_dev, threshold_type=threshold_type,
                                     cut=anomalous_cdf_at_mean_plus_1sig,
                                     win=int(1.0 / min_freq_hz * window_for_validation_Tmax))
    for t in range(n_t):
        if rejected[t]:
            out[t] = empty
            continue
        b0, b1 = bounds[t], bounds[t + 1]
        idx = merged[t]
        if remove_edges:                        # (data_buffer_sec is given: checked on entry)
            idx = idx[idx * step >= lo_edge]
            if hi_edge is not None:
                idx = idx[idx * step < hi_edge]
        if with_values:
            pos = b0 + np.searchsorted(c_index[b0:b1], idx)     # candidates come sorted by index within a row
            out[t] = (idx, c_cc[pos], c_thr[pos])
        else:
            out[t] = idx
    if timings is not None:
        timings.update(threshold_ms=(t_1 - t_0) * 1e3, candidates_ms=(t_2 - t_1) * 1e3,
                       merge_ms=(time.perf_counter() - t_2) * 1e3, candidates=int(cand.size))
    return out


def flag_multiples(origin_time_sec, template_rows, cc, pair_ok, dt_criterion=4.0, device=None, out=None):
    """The loop of ``TemplateGroup.remove_multiples`` (BPMF/dataset.py:5214-5282) on the device
    (bpmf_flag_multiples_dev, csrc/multiples.hip): which events stay `unique_event` when several templates detect the
    same event.  Arguments and result as postprocess.flag_multiples, the host definition it equals element for element:
    `origin_time_sec` (n,) float64, `template_rows` (n,) rows of `pair_ok`, `cc` (n,) float32 and finite, `pair_ok`
    (T, T) bool (postprocess.multiples_pair_mask) -- or a (T, T) uint8 / bool tensor on the GPU (template_pair_masks),
    which is read where it lies; returns an (n,) bool NumPy array in the order of the input.

    The events are visited in the stable order of their origin times (np.argsort(kind="stable"): equal times keep the
    input order, where the reference's pandas quicksort leaves the order to the platform).  One call of the library,
    which synchronises once, then the flags are scattered back to the input order.  `device`: the GPU (default: the
    current one); `out`: an optional uint8 tensor of length n on that GPU that receives the flags IN SORTED ORDER (the
    library's own output buffer, every element written)."""
    import torch
    from . import _lib
    d_ok = None
    if isinstance(pair_ok, torch.Tensor):      # a device mask (template_pair_masks) is used where it lies
        d_ok = _device_pair_mask("flag_multiples", "pair_ok", pair_ok)
        t, rows, c, ok = pp.multiples_arguments(origin_time_sec, template_rows, cc, None, n_templates=d_ok.shape[0])
        n, T = t.shape[0], d_ok.shape[0]
        if device is not None and _cuda_device("flag_multiples", device, "postprocess.flag_multiples") != d_ok.device:
            raise ValueError(f"flag_multiples: pair_ok lies on {d_ok.device}, not on {device}")
        device = d_ok.device
    else:
        t, rows, c, ok = pp.multiples_arguments(origin_time_sec, template_rows, cc, pair_ok)
        n, T = t.shape[0], ok.shape[0]
    dev = _cuda_device("flag_multiples", device, "postprocess.flag_multiples")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.shape != (n,) or
                            out.device != dev or not out.is_contiguous()):
        raise ValueError(f"flag_multiples: out must be a contiguous uint8 tensor of length {n} on {dev}")
    if n == 0:
        return np.zeros(0, dtype=bool)
    if T == 0:
        raise ValueError("flag_multiples: pair_ok is empty")
    order = np.argsort(t, kind="stable")
    d_t = torch.as_tensor(t[order], device=dev)
    d_rows = torch.as_tensor(rows[order], device=dev)
    d_cc = torch.as_tensor(c[order], device=dev)
    if d_ok is None:
        d_ok = torch.as_tensor(ok.view(np.uint8), device=dev)
    ws = torch.empty(_lib.lib().bpmf_flag_multiples_workspace_bytes(n), dtype=torch.uint8, device=dev)
    flags = torch.empty(n, dtype=torch.uint8, device=dev) if out is None else out
    _lib.call("bpmf_flag_multiples_dev", dev, d_t, d_rows, d_cc, n, d_ok, T, float(dt_criterion), ws, ws.numel(),
              _lib.STREAM, flags)
    unique = np.empty(n, dtype=bool)
    unique[order] = flags.cpu().numpy().astype(bool)
    return unique


# ------------------------------------------------------------------ pair geometry (csrc/geometry.hip) ---
def _cuda_device(name, device, definition):
    """The torch device of `device` (None: the current GPU); ValueError for anything that is not a GPU."""
    import torch
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise ValueError(f"{name}: no CPU implementation here (the host definition is {definition})")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _device_pair_mask(name, what, mask):
    """A (T, T) mask that already lies on a GPU, as the uint8 tensor the kernels read."""
    import torch
    if not mask.is_cuda or mask.dtype not in (torch.uint8, torch.bool) or mask.dim() != 2 or \
            mask.shape[0] != mask.shape[1] or mask.shape[0] == 0 or not mask.is_contiguous():
        raise ValueError(f"{name}: a tensor {what} must be a contiguous (T, T) uint8 or bool tensor on a GPU")
    return mask.view(torch.uint8)


def _geo_table(lon, lat, dep):
    """(4, n) float64: longitude, sin and cos of the reduced latitude, depth -- what the kernels read per point."""
    su, cu = pp.reduced_latitude_sin_cos(lat)
    return np.ascontiguousarray(np.stack([lon, su, cu, dep.astype(np.float64)]))


def compute_distances(src_lon, src_lat, src_dep, rcv_lon, rcv_lat, rcv_dep, return_epicentral_distances=False,
                      nonconverged="raise", device=None, *, return_metres=False, count_out=None):
    """utils.compute_distances (BPMF/utils.py:1419-1498) on the device (bpmf_geo_distances_dev, csrc/geometry.hip):
    the (K, R) float32 hypocentral distances in km between K sources and R receivers as a tensor on the GPU, and with
    `return_epicentral_distances` a tuple with the (K, R) float32 epicentral distances as well (`return_metres`: and
    the geodesic's float64 metres).  Arguments as postprocess.compute_distances_host, the definition: Vincenty's
    inverse on WGS84 in place of cartopy, the reference's roundings, float32 throughout when both depth arrays are
    float32.  The float32 results are the definition's two rounding steps applied to the device's own metres, which
    lie within a few ulp of the host's.

    nonconverged="raise" reads the 4-byte count of pairs the iteration gave up on (nearly antipodal points) and raises
    ValueError if there is any; "antipodal" gives them pi (a + b) / 2 and does not synchronise.  `count_out`: an
    optional int32 tensor of one element on the GPU that receives the count."""
    import torch
    from . import _lib
    slon, slat, sdep, rlon, rlat, rdep, depth_f64 = pp.distances_arguments(src_lon, src_lat, src_dep, rcv_lon,
                                                                           rcv_lat, rcv_dep)
    if nonconverged not in ("raise", "antipodal"):
        raise ValueError("nonconverged must be 'raise' or 'antipodal'")
    dev = _cuda_device("compute_distances", device, "postprocess.compute_distances_host")
    K, R = slon.shape[0], rlon.shape[0]
    if count_out is not None and (not isinstance(count_out, torch.Tensor) or count_out.dtype != torch.int32 or
                                  count_out.numel() != 1 or count_out.device != dev):
        raise ValueError(f"compute_distances: count_out must be an int32 tensor of one element on {dev}")
    hypo = torch.empty((K, R), dtype=torch.float32, device=dev)
    epi = torch.empty((K, R), dtype=torch.float32, device=dev) if return_epicentral_distances else None
    metres = torch.empty((K, R), dtype=torch.float64, device=dev) if return_metres else None
    if K and R:
        d_src = torch.as_tensor(_geo_table(slon, slat, sdep), device=dev)
        d_rcv = torch.as_tensor(_geo_table(rlon, rlat, rdep), device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev) if count_out is None else count_out
        _lib.call("bpmf_geo_distances_dev", dev, d_src, K, d_rcv, R, 1 if depth_f64 else 0, _lib.STREAM, hypo, epi,
                  metres, count)
        if nonconverged == "raise":
            n_bad = int(count.item())
            if n_bad:
                raise ValueError(f"compute_distances: no convergence for {n_bad} pair(s) (nearly antipodal points)")
    elif count_out is not None:
        count_out.zero_()
    out = (hypo,) + ((epi,) if epi is not None else ()) + ((metres,) if metres is not None else ())
    return out if len(out) > 1 else hypo


def template_geometry(longitude, latitude, depth, cov_mat=None, has_cov=None, depth_unit="reference", device=None):
    """The pair matrices of a TemplateGroup (BPMF/dataset.py:4568-4688) on the device (bpmf_template_geometry_dev,
    csrc/geometry.hip): a dict of `intertemplate_dist`, `dir_errors` and `ellipsoid_dist`, (T, T) float32 tensors on
    the GPU.  Arguments as postprocess.template_geometry_host, the definition, whose docstring states what is kept
    as the reference has it (Mercator metres beside depths in km; depth_unit="metres" is the alternative) and that
    the Mercator projection is restated from its documentation, not verified against cartopy.  The host projects the T
    points and uploads them; the T^2 pairs are the kernel's.  dir_errors equals the definition bit for bit, the
    distances are its roundings of the device's own geodesic, and ellipsoid_dist is the float32
    (dist - dir_errors) - dir_errors.T of the device's matrices.  No synchronisation."""
    import torch
    from . import _lib
    lon, lat, dep, xyz, cov, has = pp.template_geometry_arguments(longitude, latitude, depth, cov_mat, has_cov,
                                                                  depth_unit)
    dev = _cuda_device("template_geometry", device, "postprocess.template_geometry_host")
    T = lon.shape[0]
    d_geo = torch.as_tensor(_geo_table(lon.astype(np.float64), lat.astype(np.float64), dep), device=dev)
    d_xyz = torch.as_tensor(np.ascontiguousarray(xyz.T), device=dev)
    d_cov = d_has = None
    if cov is not None and has.any():
        # rows without a covariance are never read as numbers: they are zeroed so that nothing non-finite travels
        d_cov = torch.as_tensor(np.ascontiguousarray(np.where(has[:, None, None], cov, 0.0).reshape(T, 9).T), device=dev)
        d_has = torch.as_tensor(has.view(np.uint8), device=dev)
    out = {k: torch.empty((T, T), dtype=torch.float32, device=dev)
           for k in ("intertemplate_dist", "dir_errors", "ellipsoid_dist")}
    _lib.call("bpmf_template_geometry_dev", dev, d_geo, d_xyz, d_cov, d_has, T, _lib.STREAM, out["intertemplate_dist"],
              out["dir_errors"], out["ellipsoid_dist"], None)
    return out


def _float32_comparand(value):
    """The float64 against which a float32 matrix is compared so that the result is NumPy's for `matrix < value`: a
    Python number is weak and compares as float32, a NumPy scalar keeps its own type."""
    if isinstance(value, np.generic):
        return float(value)
    with np.errstate(over="ignore"):
        return float(np.float32(value))


def template_pair_masks(ellipsoid_dist, *, distance_criterion=None, intertemplate_cc=None, similarity_criterion=-1.0,
                        distance_threshold=None, device=None):
    """The (T, T) masks the catalogue stages read off `ellipsoid_dist`, as uint8 tensors on the GPU
    (bpmf_pair_mask_dev, csrc/geometry.hip), in a dict:
      "pair_ok"    with `distance_criterion`: postprocess.multiples_pair_mask -- ellipsoid_dist < distance_criterion,
                   and only when similarity_criterion > -1 also intertemplate_cc >= similarity_criterion -- what
                   flag_multiples takes;
      "pair_mask"  with `distance_threshold`: postprocess.intertemplate_pair_mask -- not (ellipsoid_dist[u, t] >
                   distance_threshold), the column the reference reads -- what intertemplate_cc takes.
    `ellipsoid_dist` (and `intertemplate_cc`): (T, T) float32, the GPU tensor of template_geometry as it is, or a host
    array, which is uploaded.  The comparisons are NumPy's on float32 matrices (a NaN fails both: 0 in pair_ok, 1 in
    pair_mask).  No synchronisation."""
    import torch
    from . import _lib
    if distance_criterion is None and distance_threshold is None:
        raise ValueError("template_pair_masks: give distance_criterion (pair_ok), distance_threshold (pair_mask) or both")
    want_sim = distance_criterion is not None and similarity_criterion > -1.0
    if want_sim and intertemplate_cc is None:
        raise ValueError("template_pair_masks: similarity_criterion > -1 needs intertemplate_cc")

    def square(name, x, shape=None):
        if isinstance(x, torch.Tensor):
            if x.dtype != torch.float32 or x.dim() != 2 or x.shape[0] != x.shape[1] or not x.is_cuda:
                raise ValueError(f"template_pair_masks: a tensor {name} must be (T, T) float32 on a GPU")
        else:
            x = np.asarray(x)
            if x.dtype != np.float32 or x.ndim != 2 or x.shape[0] != x.shape[1]:
                raise ValueError(f"template_pair_masks: {name} must be (T, T) float32; got {x.dtype} {x.shape}")
        if x.shape[0] == 0 or (shape is not None and tuple(x.shape) != tuple(shape)):
            raise ValueError(f"template_pair_masks: {name} has shape {tuple(x.shape)}")
        return x

    ell = square("ellipsoid_dist", ellipsoid_dist)
    sim = square("intertemplate_cc", intertemplate_cc, ell.shape) if want_sim else None
    if device is None and isinstance(ell, torch.Tensor):
        device = ell.device
    dev = _cuda_device("template_pair_masks", device, "postprocess.multiples_pair_mask / intertemplate_pair_mask")
    for name, x in (("ellipsoid_dist", ell), ("intertemplate_cc", sim)):
        if isinstance(x, torch.Tensor) and x.device != dev:
            raise ValueError(f"template_pair_masks: {name} lies on {x.device}, not on {dev}")
    d_ell = torch.as_tensor(ell, device=dev).contiguous()
    d_sim = torch.as_tensor(sim, device=dev).contiguous() if sim is not None else None
    T = d_ell.shape[0]
    jobs = []
    if distance_criterion is not None:
        jobs.append(("pair_ok", 0, distance_criterion, d_sim, similarity_criterion if want_sim else -1.0))
    if distance_threshold is not None:
        jobs.append(("pair_mask", 1, distance_threshold, None, -1.0))
    out = {}
    for key, mode, criterion, cc, similarity in jobs:
        mask = torch.empty((T, T), dtype=torch.uint8, device=dev)
        _lib.call("bpmf_pair_mask_dev", dev, d_ell, cc, T, mode, _float32_comparand(criterion),
                  _float32_comparand(similarity), _lib.STREAM, mask)
        out[key] = mask
    return out


def _detections_events(detections, *, sr, step, t0_sec):
    """The events of {template: (indices, cc, threshold)} in records_to_detections' order -- by template, then by
    index as given: (templates in that order, origin_time_sec, template_rows, cc)."""
    tids = sorted(detections)
    idx = [np.asarray(detections[t][0], dtype=np.int64).reshape(-1) for t in tids]
    rows = np.concatenate([np.full(len(i), t, dtype=np.int64) for t, i in zip(tids, idx)]) if tids else np.zeros(0, np.int64)
    index = np.concatenate(idx) if tids else np.zeros(0, np.int64)
    val = np.concatenate([np.asarray(detections[t][1], dtype=np.float32).reshape(-1) for t in tids]) if tids else \
        np.zeros(0, np.float32)
    return tids, t0_sec + index * step / sr, rows, val


def detections_unique(detections, *, sr, step, pair_ok, dt_criterion, t0_sec=0.0, device=None, on_host=False):
    """flag_multiples for the detections of a day as the sharded search returns them: `detections` = {template:
    (cc indices, cc, threshold)}, the template being the row of `pair_ok`.  origin_time_sec = t0_sec + indices * step /
    sr; the events are taken in records_to_detections' order (by template, then by index), which is therefore the
    order among equal origin times.  Returns {template: bool array} aligned with the detections.  `on_host`: through
    the host mirror (postprocess.flag_multiples) instead of the device."""
    tids, t, rows, val = _detections_events(detections, sr=sr, step=step, t0_sec=t0_sec)
    if on_host:
        unique = pp.flag_multiples(t, rows, val, pair_ok, dt_criterion)
    else:
        unique = flag_multiples(t, rows, val, pair_ok, dt_criterion, device=device)
    bounds = np.cumsum([0] + [len(detections[t][0]) for t in tids])
    return {t: unique[bounds[k]:bounds[k + 1]] for k, t in enumerate(tids)}


# ------------------------------------------------------------------ one process per GPU ---
RECORD_WIDTH = 4      # (global template id, cc index, float32 bits of cc, float32 bits of the threshold) as int64


def detections_to_records(detections, t_offset=0):
    """{row: (indices, cc, threshold)} -> (n, 4) int64 NumPy records with GLOBAL template ids."""
    rows = []
    for t in sorted(detections):
        idx, val, thr = detections[t]
        if len(idx) == 0:
            continue
        r = np.empty((len(idx), RECORD_WIDTH), dtype=np.int64)
        r[:, 0] = t + t_offset
        r[:, 1] = idx
        r[:, 2] = np.asarray(val, dtype=np.float32).view(np.int32)
        r[:, 3] = np.asarray(thr, dtype=np.float32).view(np.int32)
        rows.append(r)
    return np.concatenate(rows) if rows else np.zeros((0, RECORD_WIDTH), dtype=np.int64)


def records_to_detections(records, n_templates):
    """(n, 4) int64 records -> {template: (indices int64, cc float32, threshold float32)} for every template."""
    records = np.asarray(records, dtype=np.int64).reshape(-1, RECORD_WIDTH)
    order = np.lexsort((records[:, 1], records[:, 0]))
    records = records[order]
    out = {}
    for t in range(n_templates):
        mine = records[records[:, 0] == t]
        out[t] = (mine[:, 1].copy(), mine[:, 2].astype(np.int32).view(np.float32),
                  mine[:, 3].astype(np.int32).view(np.float32))
    return out


def sharded_matched_filter_detections(templates, moveouts, weights, data, *, group=None, device=None,
                                      engine=None, detector=None, data_src=None, balance=True, step=1,
                                      extract_peak_amplitudes=False, offset_win_peak_amp_sec=1.0,
                                      duration_win_peak_amp_sec=3.0, moveouts_peak_amp=None, data_norm=None,
                                      multiples=None, **detection_kwargs):
    """Matched-filter search of one day on ALL ranks of a torch.distributed group (one process per GPU):
    what ``MatchedFilter.run_matched_filter_search`` (BPMF/similarity_search.py:726-807) does with its
    sequential template chunks, the chunks being the ranks' shards here.

    Every rank passes the SAME templates / moveouts / weights (all T of them).  `data`: the (S, C, N) day on
    every rank, or -- with `data_src=r` -- on rank r only (None elsewhere): rank r uploads it and
    broadcasts it over RCCL / xGMI, the host of the other ranks never touches it (SURVEY.md section 8e:
    "broadcast once per day").  Rank r computes the CC of its block of templates (balanced by weighted
    channels), thresholds it and selects its detections on its own GPU (cc_detections); the (template,
    index, cc, threshold) records -- a few KB -- are all-gathered; the CC matrix never leaves the GPU
    that made it.  `detection_kwargs` are cc_detections' (sr, threshold_window_dur, ...).

    Returns (detections, info): detections = {global template id: (cc indices, cc, threshold)} for ALL
    templates, identical on every rank and equal to what matched_filter_detections(..., with values)
    finds in one process; info = {"templates": (t0, t1), "cc": this rank's CC tensor or None,
    "records_gathered": n, "broadcast_ms": float or None}.

    `extract_peak_amplitudes` (with `offset_win_peak_amp_sec`, `duration_win_peak_amp_sec`, `moveouts_peak_amp`
    (T, S, C), `data_norm`: matched_filter_detections'; needs `sr` among the detection_kwargs): every rank gathers
    the peak amplitudes of ITS templates' detections from the day on its own GPU (peak_amplitudes) -- with
    `data_src` the only place a rank other than the source can read the day from -- and a second all-gather of
    (n, S * C) float32 rows brings them together: info["peak_amplitudes"] = {global template id: (n, S, C)},
    identical on every rank and ordered like the returned detections.

    `multiples` = dict(pair_ok=(T, T) bool, dt_criterion=seconds, t0_sec=0.0) (needs `sr` among the
    detection_kwargs): after the all-gather every rank flags the events several templates detected
    (``TemplateGroup.remove_multiples``, BPMF/dataset.py:5130-5295; detections_unique) -- the same records in the same
    order on every rank, hence the same flags: info["unique_event"] = {global template id: bool array} aligned with the
    returned detections.  On this rank's GPU, or through the host mirror when the engine's day is not on one.

    `engine` / `detector`: stand-ins for the per-rank MatchedFilterGPU and for cc_detections (the CPU tests
    of the choreography over gloo pass oracle-backed ones); None = the HIP path.  An engine whose day (`.data`) is not
    on a GPU gets its amplitudes from the host mirror, postprocess.peak_amplitudes_host.

    threshold_type="mad" needs an explicit `white_noise` here: without one every rank would draw its own
    (np.random, as the reference does per call) and the ranks' detections would not be those of one process."""
    import time
    import torch
    from . import parallel
    if detector is None and str(detection_kwargs.get("threshold_type", "rms")).lower() == "mad" and \
            detection_kwargs.get("white_noise") is None:
        raise ValueError("sharded_matched_filter_detections: threshold_type='mad' needs white_noise (the same array on "
                         "every rank); each rank would otherwise draw its own")
    smf = parallel.ShardedMatchedFilter(group=group, device=device, local=engine)
    t_b = None
    if data_src is None:
        smf.set_data(data)
    else:
        t0c = time.perf_counter()
        smf.set_data_broadcast(data, src=data_src)
        t_b = (time.perf_counter() - t0c) * 1e3
    weights = np.asarray(weights, dtype=np.float32)
    T = weights.shape[0]
    t0, t1, cc = smf.run(templates, moveouts, weights, step, True, balance=balance)
    if cc is None:
        mine = {}
    elif detector is not None:
        mine = detector(cc, np.asarray(moveouts)[t0:t1], weights[t0:t1], step=step, **detection_kwargs)
    else:
        mine = cc_detections(cc, np.asarray(moveouts)[t0:t1], weights[t0:t1], step=step, device=device,
                             with_values=True, **detection_kwargs)
    rec = detections_to_records(mine, t_offset=t0)
    rec_dev = smf.record_device()
    parts = parallel.allgather_varlen(torch.as_tensor(rec, device=rec_dev), group=group)
    everything = np.concatenate([p.cpu().numpy() for p in parts]) if parts else rec
    info = {"templates": (t0, t1), "cc": cc, "records_gathered": int(everything.shape[0]), "broadcast_ms": t_b}
    if extract_peak_amplitudes:
        if "sr" not in detection_kwargs:
            raise ValueError("sharded_matched_filter_detections: extract_peak_amplitudes needs sr")
        offset, duration = _peak_amplitude_window(detection_kwargs["sr"], offset_win_peak_amp_sec,
                                                  duration_win_peak_amp_sec)
        mv_amp = np.asarray(moveouts if moveouts_peak_amp is None else moveouts_peak_amp)
        day = smf.local.data
        # this rank's records carry global template ids, in the order they are gathered in
        gather = peak_amplitudes if isinstance(day, torch.Tensor) and day.is_cuda else pp.peak_amplitudes_host
        amp = gather(day, rec[:, 0], rec[:, 1] * step, mv_amp, offset=offset, duration=duration, data_norm=data_norm)
        n_chan = int(np.prod(amp.shape[1:]))
        parts = parallel.allgather_varlen(torch.as_tensor(amp.reshape(len(rec), n_chan), device=rec_dev), group=group)
        amp_all = np.concatenate([p.cpu().numpy() for p in parts]).reshape((-1,) + amp.shape[1:])
        order = np.lexsort((everything[:, 1], everything[:, 0]))              # records_to_detections' order
        info["peak_amplitudes"] = _split_by_row(everything[order, 0], amp_all[order], T)
    found = records_to_detections(everything, T)
    if multiples is not None:
        if "sr" not in detection_kwargs:
            raise ValueError("sharded_matched_filter_detections: multiples needs sr")
        day = smf.local.data
        on_gpu = isinstance(day, torch.Tensor) and day.is_cuda
        info["unique_event"] = detections_unique(found, sr=detection_kwargs["sr"], step=step,
                                                 pair_ok=multiples["pair_ok"], dt_criterion=multiples["dt_criterion"],
                                                 t0_sec=multiples.get("t0_sec", 0.0),
                                                 device=day.device if on_gpu else None, on_host=not on_gpu)
    return found, info


def sharded_backprojection_detections(features, moveouts, weights_phases, weights_sources, *, sr,
                                      minimum_interevent_time, threshold_window_dur=None, n_dev=15.0,
                                      overlap=0.75, threshold=None, out_of_bounds="strict", group=None,
                                      device=None, engine_factory=None, detector=None, features_src=None):
    """Backprojection of one day with the source grid tiled over the ranks of a group: every rank scans
    its block of sources (global ids) against the whole day of features, ONE all-reduce(MAX) of packed
    (beam, id) keys leaves the global max-beam and arg-max on every rank (ties -> the lowest source id,
    as one sequential scan), and every rank runs the (3 ms) detection stage on them.  Mirrors
    ``Beamformer.backproject`` + ``find_detections`` (BPMF/template_search.py:508-627).

    `features`: the (S, C, N) day on every rank, or with `features_src=r` on rank r only (broadcast over
    the group).  Returns (peak samples, source indices, maxbeam, argmax) -- the tensors of
    backprojection_detections(return_device=True) -- identical on every rank.
    `engine_factory(moveouts_block, weights_block, source_id_offset)` / `detector(beam, arg)`: CPU
    stand-ins for BeamformerGPU / beam_detections_device in the gloo tests."""
    from . import parallel
    sb = parallel.ShardedBeamformer(moveouts, weights_sources, group=group, device=device,
                                    local_factory=engine_factory)
    try:                                 # (the per-rank engine -- plan and working set -- goes whatever happens)
        if features_src is not None:
            features = sb.broadcast_features(features, src=features_src)
        beam, arg = sb.run(features, weights_phases, "max", out_of_bounds)
        mpd = int(pp.sec_to_samp(minimum_interevent_time, sr))
        if detector is not None:
            peaks, peak_sources = detector(beam, arg)
        else:
            window = None if threshold is not None else int(pp.sec_to_samp(threshold_window_dur, sr))
            peaks, peak_sources, _ = beam_detections_device(beam, arg, mpd=mpd, threshold=threshold, window=window,
                                                           n_dev=n_dev, overlap=overlap, device=device)
    finally:
        sb.close()
    return peaks, peak_sources, beam, arg


def beam_detections_device(beam, arg, *, mpd, threshold=None, window=None, n_dev=15.0, overlap=0.75,
                           device=None, detector=None):
    """``Beamformer.find_detections`` (BPMF/template_search.py:574-627) on a max-beam that lives
    on the device: `beam` (N,) float32 and `arg` (N,) int32 device tensors (the output of
    BeamformerGPU.run).  Nothing of length N is downloaded:

      1. threshold: per-window median / MAD by radix select on the device (csrc/bp_detect.hip),
         n_windows + 2 node values to the host (`threshold` None), or a scalar given by the caller;
      2. the rising-edge local maxima above the smallest threshold node, compacted on the device;
      3. on that list: tallest-first min-distance suppression, the float64 threshold test at the
         survivors, the +-mpd/2 snap (on windows of the beam gathered in one small transfer) and
         np.unique -- the reference's own index logic (postprocess.find_beam_detections_from_candidates).

    The result is postprocess.find_beam_detections on the downloaded series for every float32 series, +-Inf
    included (DESIGN.md s4 "Non-finite features", rule 3), and for every form of the threshold.

    `detector`: an object with ``window_stats(beam, window, overlap)`` and ``extract_peaks(beam, sources, floor)``
    in place of a threshold.BeamDetectorGPU -- the CPU stand-in of the host tests; everything else here works
    on CPU tensors as well.

    Returns (peak samples int64, source indices int32, threshold nodes (centre, values) or None)."""
    import torch
    if detector is None:
        from .threshold import BeamDetectorGPU
        detector = BeamDetectorGPU(device=device if device is not None else beam.device.index)
    det = detector
    n = beam.numel()
    nodes = None
    if threshold is None:
        med, mad = det.window_stats(beam, window, overlap)
        centre, thr = pp.bp_threshold_nodes(n, int(window), overlap, med, mad, n_dev)
        nodes = (centre, thr)
        # a NaN node (a window that holds a NaN, or the reference's empty last window when the
        # series is a whole number of non-overlapping windows) makes the interpolated threshold
        # NaN around it, where the reference then keeps no peak (`>` is false); the floor is the
        # smallest node that is not NaN (a +Inf node -- a finite median under an Inf MAD -- lets nothing pass around
        # it either) -- less one float32 ulp: the interpolation (SciPy's order of operations,
        # pp.interp_threshold) can land an ulp of float64 below two equal nodes, and a peak exactly as high
        # as the node would then pass the reference's `>` but not the floor
        real = thr[~np.isnan(thr)]
        floor = float(np.nextafter(np.float32(real.min()), np.float32(-np.inf))) if real.size else float("nan")

        def threshold_at(samples):
            return pp.interp_threshold(samples, centre, thr)
    elif np.ndim(threshold) == 0:
        floor = float(threshold)

        def threshold_at(samples):
            return np.full(len(samples), float(threshold))
    else:
        thr_arr = np.asarray(threshold)
        real = thr_arr[~np.isnan(thr_arr)]
        floor = float(real.min()) if real.size else float("nan")

        def threshold_at(samples):
            return thr_arr[samples]
    # a NaN floor (no threshold value that is not NaN) or a +Inf one: nothing can exceed it.  A -Inf floor is a
    # threshold like any other: every peak is above it, as in the reference (`x > -inf`)
    if np.isnan(floor) or floor == np.inf:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32), nodes
    rec = det.extract_peaks(beam, arg, floor)
    if mpd > 1 and pp.has_close_ties(rec["index"], rec["beam"], mpd):
        # two exactly equal peaks closer than mpd: which one survives depends on where NumPy's
        # unstable sort puts them in the list of ALL local maxima (pp._tallest_first) -- fetch that
        # list (12 bytes per local maximum; rare on real beams, common on rounded test series)
        rec = det.extract_peaks(beam, arg, -np.inf)
    # beam windows around every candidate that can survive, in ONE gather + transfer: the snap
    # looks +-mpd/2 around a peak, and a snapped peak can be looked at once more (+-mpd covers it)
    half = int(mpd) + 1
    idx_all = rec["index"].astype(np.int64)
    cache = {}
    if idx_all.size:
        keep_rank = pp._tallest_first(rec["beam"].astype(np.float64))
        keep = pp._suppress(idx_all, keep_rank, mpd) if mpd > 1 else np.ones(idx_all.size, bool)
        cand = idx_all[keep]
        cand = cand[rec["beam"][keep].astype(np.float64) > threshold_at(cand)]
        if cand.size:
            offs = torch.arange(-half, half + 1, device=beam.device)
            pos = (torch.as_tensor(cand, device=beam.device)[:, None] + offs[None, :]).clamp_(0, n - 1)
            wins = beam.reshape(-1)[pos].cpu().numpy()
            for c, wrow in zip(cand, wins):
                cache[int(c)] = wrow
    flat = beam.reshape(-1)

    centres = np.array(sorted(cache), dtype=np.int64)     # a busy day has thousands of candidates: bisect

    def beam_slice(i0, i1):
        # a gathered window [c - half, c + half] that covers [i0, i1): c in [i1 - 1 - half, i0 + half]
        j = int(np.searchsorted(centres, i1 - 1 - half, side="left"))
        while j < centres.size and centres[j] <= i0 + half:
            c = int(centres[j])
            lo = c - half
            if lo >= 0 and c + half < n:         # windows clamped at the ends of the trace are not contiguous
                return cache[c][i0 - lo:i1 - lo]
            j += 1
        return flat[i0:i1].cpu().numpy()         # rare: a window no candidate's gather covers

    peaks = pp.find_beam_detections_from_candidates(idx_all, rec["beam"], threshold_at, mpd, n, beam_slice)
    if peaks.size:
        src = arg.reshape(-1)[torch.as_tensor(peaks, device=arg.device)].cpu().numpy()
    else:
        src = np.zeros(0, dtype=np.int32)
    return peaks, src, nodes


_FOCUS_BLOCK = 1 << 22      # elements of the volume scanned per step of _first_maximum


def _first_maximum(vol):
    """(src_idx, time_idx) of the point of maximum focusing of a (K, N) beam volume on the device: the first maximum in
    source-major order among the beams that are not NaN -- a NaN beam is never the maximum and +Inf is, the rule of the
    running maximum behind reduce="max" (DESIGN.md s4 "Non-finite features"); (0, 0) for a volume of nothing but NaN.
    On a volume without NaN this is np.unravel_index(vol.argmax(), vol.shape).  Scanned in blocks of whole rows, so the
    only temporaries are block-sized; one synchronisation."""
    import torch
    K, N = vol.shape
    rows = max(1, _FOCUS_BLOCK // N)
    best, where = [], []
    for k0 in range(0, K, rows):
        part = vol[k0:k0 + rows].reshape(-1)
        part = torch.where(part != part, float("-inf"), part)
        i = torch.argmax(part)                   # the first maximum of the block
        best.append(part[i])
        where.append(i + k0 * N)
    first = int(torch.stack(where)[torch.argmax(torch.stack(best))])      # the first block that reaches the maximum
    return divmod(first, N)


def relocation_focus(beamformer, features, weights_phases, uncertainty_method="spatial",
                     out_of_bounds="flexible"):
    """The beamforming step of the reference's event relocation, ``Event.relocate_beam``
    (BPMF/dataset.py:2186-2216), on a resident BeamformerGPU: the short feature array of one event
    (N ~ 1 500-3 000 samples) is backprojected over the whole grid and the point of maximum focusing
    is found on the device.

    "spatial" (``reduce="none"``): the (K, N) beam volume stays in HBM; returns
    ``(src_idx, time_idx, beam[:, time_idx])`` -- np.unravel_index(beam.argmax(), beam.shape), i.e.
    the first maximum in source-major order, and the column the reference turns into its location
    likelihood (K floats downloaded instead of K*N).  "temporal" (``reduce="max"``): returns
    ``(src_idx, time_idx, maxbeam)`` with time_idx = maxbeam.argmax() (first maximum) and
    src_idx = maxbeam_sources[time_idx].  `out_of_bounds` defaults to the reference's "flexible"
    (:2186).

    Non-finite features: a NaN beam is never the maximum and a +Inf beam is, under both methods (the max-beam
    of "temporal" is never NaN).  The reference's np.argmax stops at the first NaN of a volume that holds one;
    that is deliberately not followed -- a focus on a NaN is useless, and it is what relocate_events and the
    reference's own "temporal" method return.  The column comes back as it is, NaN beams included."""
    import torch
    if uncertainty_method == "spatial":
        vol = beamformer.run(features, weights_phases, "none", out_of_bounds)        # (K, N) on the device
        src_idx, time_idx = _first_maximum(vol)
        return src_idx, time_idx, vol[:, time_idx].cpu().numpy()
    if uncertainty_method == "temporal":
        beam, arg = beamformer.run(features, weights_phases, "max", out_of_bounds)
        time_idx = int(torch.argmax(beam))
        return int(arg[time_idx]), time_idx, beam.cpu().numpy()
    raise ValueError("uncertainty_method should be 'spatial' or 'temporal'")


def _likelihood_of_column(col):
    """postprocess.likelihood on a device column: float32 subtract / divide / clip; a NaN in the column makes min and
    max NaN and with them the whole row, as np.min / np.max do."""
    lo, hi = col.min(), col.max()
    return ((col - lo) / (hi - lo)).clamp_(0.0, 1.0)


def relocation_likelihood(beamformer, features, weights_phases, out_of_bounds="flexible", domain=None):
    """The spatial branch of ``Event.relocate_beam`` (BPMF/dataset.py:2186-2245) up to the likelihood,
    on the device: backprojection of the event's short feature array over the whole grid
    (``reduce="none"``, the (K, N) volume stays in HBM), the point of maximum focusing, and
    ``Beamformer._likelihood`` of the beam column at that time (BPMF/template_search.py:498-506) --
    float32 subtract / divide / clip, the operations NumPy performs, evaluated on the column where it
    lies.  Only `likelihood[domain]` (or the whole (K,) vector when `domain` is None) comes back.

    Non-finite features: the focus is relocation_focus's (a NaN beam is never the maximum, +Inf is; the
    reference's np.argmax on a volume with a NaN is deliberately not followed).  A NaN in the column makes the
    whole likelihood NaN; an Inf maximum gives 0 on the finite entries and NaN at the Inf -- what
    postprocess.likelihood gives for that column.

    Returns (src_idx, time_idx, likelihood): feed `likelihood` and the domain's coordinates to
    postprocess.compute_location_uncertainty for (hunc, vunc)."""
    import torch
    vol = beamformer.run(features, weights_phases, "none", out_of_bounds)
    src_idx, time_idx = _first_maximum(vol)
    like = _likelihood_of_column(vol[:, time_idx])
    if domain is not None:
        like = like[torch.as_tensor(np.asarray(domain, dtype=np.int64), device=like.device)]
    return src_idx, time_idx, like.cpu().numpy()


def _relocation_windows(features, starts, n_samples):
    """Shapes of relocate_events' input, checked without touching a device: (E, S, C, N, starts int64 or None)."""
    shape = tuple(features.shape) if hasattr(features, "shape") else np.shape(features)
    if starts is None:
        if n_samples is not None:
            raise ValueError("n_samples goes with starts (windows of a day); a batch (E, S, C, N) carries its own")
        if len(shape) != 4:
            raise ValueError("features must be (E, S, C, N), one window per event -- or (S, C, N_day) with "
                             f"starts and n_samples; got {shape}")
        E, S, Cc, N = shape
        if N < 1:
            raise ValueError("windows of no samples")
        return E, S, Cc, N, None
    if n_samples is None:
        raise ValueError("starts needs n_samples, the length of every window")
    if len(shape) != 3:
        raise ValueError(f"with starts, features must be the day (S, C, N_day); got {shape}")
    st = np.asarray(starts.cpu() if hasattr(starts, "cpu") else starts)
    if st.ndim != 1 or (st.size and not np.issubdtype(st.dtype, np.integer)):
        raise ValueError("starts must be a vector of E integer sample indices")
    st = st.astype(np.int64)
    S, Cc, n_day = shape
    N = int(n_samples)
    if N < 1:
        raise ValueError("n_samples must be at least 1")
    if st.size and (st.min() < 0 or st.max() + N > n_day):
        bad = int(np.flatnonzero((st < 0) | (st + N > n_day))[0])
        raise ValueError(f"window {bad} = [{int(st[bad])}, {int(st[bad]) + N}) leaves the day of {n_day} samples "
                         "(no wrap, no clipping)")
    return st.size, S, Cc, N, st


def location_uncertainties_host(result, longitude, latitude, depth, uncertainty_method="spatial",
                                source_id_offset=0, restricted_domain_side_km=100.0, effective_kT=0.33,
                                gibbs_cutoff=0.25):
    """The end of ``Event.relocate_beam`` (BPMF/dataset.py:2207-2245) for every event of a relocate_events
    `result`, one after the other on the host -- the loop a user of relocate_events(uncertainties=False) writes,
    and the yardstick of relocate_events(uncertainties=True).  `longitude`, `latitude`, `depth`: (K,) coordinates
    of the plan's source rows.  Per event:
      "spatial":  postprocess.rectangular_domain around the new epicentre, likelihood[e][domain],
                  postprocess.compute_location_uncertainty;
      "temporal": postprocess.gibbs_weights of maxbeam[e], the samples with a weight > gibbs_cutoff, their
                  maxbeam_sources (minus `source_id_offset`) as the domain (dataset.py:2218-2227).
    Device tensors of `result` are downloaded here.  Returns a dict of (E,) arrays: longitude, latitude, depth,
    hunc, vunc (float64), n_domain (int64), and for "spatial" ``domain`` (E, K) bool."""
    from . import postprocess as pp
    if uncertainty_method not in ("spatial", "temporal"):
        raise ValueError("uncertainty_method should be 'spatial' or 'temporal'")
    spatial = uncertainty_method == "spatial"

    def host(x):
        return np.asarray(x.cpu() if hasattr(x, "cpu") else x)

    lon, lat, dep = (np.asarray(x, dtype=np.float64) for x in (longitude, latitude, depth))
    src = np.asarray(result["src_idx"], dtype=np.int64) - (0 if spatial else int(source_id_offset))
    E = src.shape[0]
    out = {k: np.zeros(E, np.float64) for k in ("longitude", "latitude", "depth", "hunc", "vunc")}
    out["n_domain"] = np.zeros(E, np.int64)
    if spatial:
        like = host(result["likelihood"])
        out["domain"] = np.zeros((E, lon.shape[0]), dtype=bool)
    else:
        maxbeam, sources = host(result["maxbeam"]), host(result["maxbeam_sources"])
    for e in range(E):
        lon0, lat0, dep0 = lon[src[e]], lat[src[e]], dep[src[e]]
        if spatial:
            domain = pp.rectangular_domain(lon0, lat0, lon, lat, side_km=restricted_domain_side_km)
            weights = like[e][domain]
            out["domain"][e] = domain
        else:
            gibbs = pp.gibbs_weights(maxbeam[e], effective_kT)
            mask = gibbs > gibbs_cutoff
            domain = sources[e][mask].astype(np.int64) - int(source_id_offset)
            weights = gibbs[mask]
        with np.errstate(invalid="ignore", divide="ignore"):
            hunc, vunc = pp.compute_location_uncertainty(lon0, lat0, dep0, weights, lon[domain], lat[domain],
                                                         dep[domain])
        out["longitude"][e], out["latitude"][e], out["depth"][e] = lon0, lat0, dep0
        out["hunc"][e], out["vunc"][e], out["n_domain"][e] = hunc, vunc, weights.shape[0]
    return out


def _uncertainty_arguments(beamformer, uncertainty_method, restricted_domain_side_km, effective_kT, gibbs_cutoff,
                           domain_mask):
    """Checks of relocate_events(uncertainties=True), made before anything touches a device."""
    if getattr(beamformer, "_coord_tables", None) is None:
        raise ValueError("uncertainties=True needs the coordinates of the sources: call "
                         "beamformer.set_source_coordinates(longitude, latitude, depth) first")
    if uncertainty_method == "spatial":
        if not (np.isfinite(restricted_domain_side_km) and restricted_domain_side_km > 0):
            raise ValueError("restricted_domain_side_km must be a positive number of kilometres")
    else:
        if domain_mask:
            raise ValueError("domain_mask belongs to the spatial method (the temporal domain is a list of samples)")
        if not (np.isfinite(effective_kT) and np.float32(effective_kT) > 0):
            raise ValueError("effective_kT must be positive")
        if not np.isfinite(gibbs_cutoff):
            raise ValueError("gibbs_cutoff must be finite")


def relocate_events(beamformer, features, weights_phases, uncertainty_method="spatial",
                    out_of_bounds="flexible", starts=None, n_samples=None, columns=False, _chunk=None,
                    uncertainties=False, restricted_domain_side_km=100.0, effective_kT=0.33, gibbs_cutoff=0.25,
                    domain_mask=False):
    """The beamforming step of ``Event.relocate_beam`` (BPMF/dataset.py:2186-2245) for a BATCH of events in one
    call on a resident BeamformerGPU -- what tutorial notebook 6 does in a loop over every detected event, and
    what relocation_focus / relocation_likelihood do for one.  The events share the launches
    (bpmf_bp_relocate_batch_dev, csrc/bp_relocate.hip): their tiles fill the chip as a day's do, the (K, N)
    volume of an event is never made, and the host synchronises once.

    `features`: (E, S, C, N), one window per event (array or device tensor) -- or the day (S, C, N_day) with
    `starts` (E first samples) and `n_samples`: event e is features[:, :, starts[e]:starts[e] + n_samples], read
    where the day lies in HBM (what backprojection_detections(..., return_device=True) leaves there).  A window
    that leaves the day raises ValueError.

    Returns a dict: ``src_idx`` (E,) int64, ``time_idx`` (E,) int64, ``max_beam`` (E,) float32 on the host, and
      "spatial":  ``likelihood`` (E, K) float32 DEVICE tensor, row e = Beamformer._likelihood of
                  beam_e[:, time_idx[e]] (NaN row for a constant column); columns=True adds ``columns``, the raw
                  beam columns.
      "temporal": ``maxbeam`` (E, N) float32 and ``maxbeam_sources`` (E, N) int32 device tensors;
                  time_idx[e] = maxbeam[e].argmax(), src_idx[e] = maxbeam_sources[e, time_idx[e]].
    For every event the result is what relocation_focus / relocation_likelihood return for it alone, bit for
    bit, ties included (first maximum in source-major order).  An event whose maximum is not > 0 although its
    window is not all zero (negative features or weights, or nothing but NaN beams) is redone on its volume by
    the per-event path.  Non-finite features: a NaN beam is never the maximum and +Inf is, the
    max-beams are never NaN; the reference's np.argmax on a volume with a NaN is deliberately not followed.  A
    NaN in the column at the focus makes the event's likelihood row NaN, an Inf maximum gives 0 on the finite
    entries and NaN at the Inf.  (``uncertainties=True`` on such a row is not defined.)
    Events run in chunks sized from the free device memory; the results do not depend on the chunks.

    ``uncertainties=True`` finishes ``Event.relocate_beam`` (dataset.py:2207-2245) in the same call, on the device
    (bpmf_bp_location_uncertainty_dev, csrc/bp_uncertainty.hip, per chunk behind the likelihood -- or the focus
    for "temporal" -- on the same stream; still one synchronisation).  The beamformer needs its sources'
    coordinates (``set_source_coordinates``), else ValueError.  The dict gains HOST arrays (E,): ``longitude``,
    ``latitude``, ``depth`` of the new hypocentre, ``hunc`` and ``vunc`` in km (float64) -- the event's
    hmax_unc = hmin_unc = hunc, vmax_unc = vunc -- and ``n_domain`` (int64), the number of sources (samples) they
    average over: "spatial" the rectangle of `restricted_domain_side_km` around the epicentre
    (postprocess.rectangular_domain, the same booleans), weighted by the likelihood; "temporal" the samples whose
    Gibbs weight exp(-(max - maxbeam) / effective_kT) exceeds `gibbs_cutoff`.  ``domain_mask=True`` ("spatial")
    adds ``domain``, the (E, K) bool device tensor of the rectangles.  location_uncertainties_host is the same
    on the host, event by event: n_domain and the rectangles are equal, hunc and vunc agree to about 1e-14 km
    (the numerators are float64 sums in a fixed order that does not depend on the batch; the denominator is the
    reference's np.sum of the float32 weights, a float32 sum in NumPy's order, reproduced bit for bit).
    With ``uncertainties=False`` the call is what it was: same launches, same keys."""
    if uncertainty_method not in ("spatial", "temporal"):
        raise ValueError("uncertainty_method should be 'spatial' or 'temporal'")
    if out_of_bounds not in ("strict", "flexible"):
        raise ValueError("out_of_bounds should be 'strict' or 'flexible'")
    if uncertainties:
        _uncertainty_arguments(beamformer, uncertainty_method, restricted_domain_side_km, effective_kT,
                               gibbs_cutoff, domain_mask)
    E, S, Cc, N, st = _relocation_windows(features, starts, n_samples)
    bf = beamformer
    if S != bf.S:
        raise ValueError("features and moveouts disagree on the number of stations")
    if tuple(np.shape(weights_phases)) != (S, Cc, bf.P):
        raise ValueError(f"weights_phases must be ({S}, {Cc}, {bf.P})")
    t = bf.torch
    dev = bf.device
    spatial = uncertainty_method == "spatial"
    K = bf.K
    time_idx = t.empty(E, dtype=t.int32, device=dev)
    src_idx = t.empty(E, dtype=t.int32, device=dev)
    max_beam = t.empty(E, dtype=t.float32, device=dev)
    like = t.empty((E, K), dtype=t.float32, device=dev) if spatial else None
    cols = t.empty((E, K), dtype=t.float32, device=dev) if spatial and columns else None
    mbeam = None if spatial else t.empty((E, N), dtype=t.float32, device=dev)
    marg = None if spatial else t.empty((E, N), dtype=t.int32, device=dev)
    res = {"src_idx": np.zeros(E, np.int64), "time_idx": np.zeros(E, np.int64), "max_beam": np.zeros(E, np.float32)}
    res.update({"likelihood": like} if spatial else {"maxbeam": mbeam, "maxbeam_sources": marg})
    if cols is not None:
        res["columns"] = cols
    unc = unc_n = dmask = unc_ws = None
    if uncertainties:
        unc = t.empty((5, E), dtype=t.float64, device=dev)     # hunc, vunc, longitude, latitude, depth
        unc_n = t.empty(E, dtype=t.int32, device=dev)
        dmask = t.empty((E, K), dtype=t.bool, device=dev) if spatial and domain_mask else None
        unc_kw = dict(side_km=restricted_domain_side_km, effective_kT=effective_kT, gibbs_cutoff=gibbs_cutoff)

        def unpack():
            host = unc.cpu().numpy()
            res.update(hunc=host[0].copy(), vunc=host[1].copy(), longitude=host[2].copy(), latitude=host[3].copy(),
                       depth=host[4].copy(), n_domain=unc_n.cpu().numpy().astype(np.int64))
            if dmask is not None:
                res["domain"] = dmask

        if E == 0:
            unpack()
    if E == 0:
        return res
    wp = bf._dev(weights_phases, t.float32)
    resident = isinstance(features, t.Tensor) and features.device == dev
    day = bf._dev(features, t.float32) if st is not None else None
    st_dev = None if st is None else t.as_tensor(st, device=dev)
    # events per launch: a quarter of the free memory for the prestacks (S P N floats per event) and the rows
    # behind them, at most the 65535 of a launch
    if _chunk is None:
        free = t.cuda.mem_get_info(dev)[0]
        per_event = (S * bf.P * N + 4 * N) * 4 + (0 if resident or st is not None else S * Cc * N * 4)
        if uncertainties:                     # the compacted weights of the event's domain
            per_event += (K if spatial else N) * 4
        _chunk = max(1, (free // 4) // per_event)
    chunk = int(max(1, min(_chunk, E, 65535)))
    ws = t.empty(max(bf.relocation_workspace_bytes(min(chunk, E - e0), N, Cc) for e0 in range(0, E, chunk)),
                 dtype=t.uint8, device=dev)
    if uncertainties:
        unc_ws = t.empty(bf.uncertainty_workspace_bytes(chunk, K if spatial else N), dtype=t.uint8, device=dev)

    def part(x, e0, e1):
        return None if x is None else x[e0:e1]

    for e0 in range(0, E, chunk):
        e1 = min(E, e0 + chunk)
        if st is not None:
            f, ev_stride, row_stride, sd = day, 0, day.shape[2], st_dev[e0:e1]
        else:
            f, ev_stride, row_stride, sd = bf._dev(features[e0:e1], t.float32), S * Cc * N, N, None
        bf.relocate_batch(f, ev_stride, row_stride, sd, wp, e1 - e0, N, Cc, out_of_bounds, uncertainty_method, ws,
                          time_idx[e0:e1], src_idx[e0:e1], max_beam[e0:e1], part(like, e0, e1), part(cols, e0, e1),
                          part(mbeam, e0, e1), part(marg, e0, e1))
        if uncertainties:
            bf.location_uncertainty(uncertainty_method, e1 - e0, N, src_idx[e0:e1], unc_ws, unc[:, e0:e1],
                                    unc_n[e0:e1], likelihood=part(like, e0, e1), maxbeam=part(mbeam, e0, e1),
                                    maxbeam_sources=part(marg, e0, e1), max_beam=max_beam[e0:e1],
                                    domain_mask=part(dmask, e0, e1), **unc_kw)
    del ws
    res["time_idx"] = time_idx.cpu().numpy().astype(np.int64)          # (the one synchronisation of the batch)
    res["src_idx"] = src_idx.cpu().numpy().astype(np.int64)
    res["max_beam"] = max_beam.cpu().numpy()
    if uncertainties:
        unpack()
    if not spatial:
        return res
    res["src_idx"] -= bf.source_id_offset          # rows of the volume, as np.unravel_index gives them
    # A maximum that is not > 0: the running maximum starts at (0, first source), so a volume whose largest
    # beam is 0 or negative does not show in the max-beam where its first maximum lies.  All-zero windows give
    # an all-zero volume, whose first maximum is (0, 0) as found; anything else goes through its volume.
    redone = False
    for e in np.flatnonzero(~(res["max_beam"] > 0)):
        e = int(e)
        win = day[:, :, int(st[e]):int(st[e]) + N] if st is not None else bf._dev(features[e], t.float32)
        if not bool((win != 0).any()):
            continue
        vol = bf.run(win.contiguous(), wp, "none", out_of_bounds)
        k, ti = _first_maximum(vol)
        col = vol[:, ti]
        like[e] = _likelihood_of_column(col)
        if cols is not None:
            cols[e] = col
        res["src_idx"][e], res["time_idx"][e], res["max_beam"][e] = k, ti, float(col[k])
        del vol
        if uncertainties:                    # from the corrected row and likelihood
            src_idx[e] = k + bf.source_id_offset
            bf.location_uncertainty("spatial", 1, N, src_idx[e:e + 1], unc_ws, unc[:, e:e + 1], unc_n[e:e + 1],
                                    likelihood=like[e:e + 1], domain_mask=part(dmask, e, e + 1), **unc_kw)
            redone = True
    if uncertainties and redone:
        unpack()
    return res


def backprojection_detections(features, moveouts, weights_phases, weights_sources, *, sr,
                              minimum_interevent_time, threshold_window_dur=None, n_dev=15.0,
                              overlap=0.75, threshold=None, out_of_bounds="strict", device=None,
                              return_device=False):
    """Backprojection of one day: returns (peak samples, source indices, maxbeam, argmax).

    The max-beam and its arg-max stay on the device through the whole detection stage
    (beam_detections_device); they are downloaded at the end only because this function returns
    them as arrays -- pass return_device=True to get the device tensors instead."""
    bf = BeamformerGPU(moveouts, weights_sources, device=device)
    beam, arg = bf.run(features, weights_phases, "max", out_of_bounds)
    mpd = int(pp.sec_to_samp(minimum_interevent_time, sr))
    window = None if threshold is not None else int(pp.sec_to_samp(threshold_window_dur, sr))
    peaks, peak_sources, _ = beam_detections_device(beam, arg, mpd=mpd, threshold=threshold,
                                                   window=window, n_dev=n_dev, overlap=overlap,
                                                   device=device)
    bf.close()
    if return_device:
        return peaks, peak_sources, beam, arg
    return peaks, peak_sources, beam.cpu().numpy(), arg.cpu().numpy()


def numpy_order_sum(x):
    """Sum over the last axis of a torch tensor in the order of numpy's float32 pairwise
    `np.sum` (n < 8: running sum; n <= 128: eight strided partial sums combined as a tree, then
    the tail; larger: split in halves of multiples of 8) -- element-wise adds only, so the
    result is bit-identical to `np.sum(a, axis=(-1, -2))` of the reference
    (dataset.py:4828-4830) whatever the device."""
    n = x.shape[-1]
    if n < 8:
        res = x.new_zeros(x.shape[:-1])
        for i in range(n):
            res = res + x[..., i]
        return res
    if n <= 128:
        r = [x[..., j] for j in range(8)]
        m = n - (n % 8)
        for i in range(8, m, 8):
            r = [r[j] + x[..., i + j] for j in range(8)]
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for i in range(m, n):
            res = res + x[..., i]
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return numpy_order_sum(x[..., :n2]) + numpy_order_sum(x[..., n2:])


def factorise_pair_weights(weights):
    """(T, T, S, C) weights -> (base (T, S, C), mask (T, T) bool) if, for every t, all non-zero rows
    weights[t, u] are one and the same (S, C) pattern -- how the reference builds them
    (dataset.py:4789-4816: template t's normalised station weights, zeroed for the templates beyond
    the distance threshold); None otherwise."""
    w = np.asarray(weights, dtype=np.float32)
    T = w.shape[0]
    mask = (w != 0).reshape(T, T, -1).any(axis=2)
    base = np.zeros((T,) + w.shape[2:], dtype=np.float32)
    for t in range(T):
        rows = np.flatnonzero(mask[t])
        if rows.size == 0:
            continue
        base[t] = w[t, rows[0]]
        if not np.array_equal(w[t, rows], np.broadcast_to(base[t], (rows.size,) + base[t].shape)):
            return None
    return base, mask


INTERTP_MAX_LAG = 31                 # the batched kernel keeps 2 * max_lag + 1 <= 63 lags per pair
INTERTP_LDS_BYTES = 64 * 1024        # ... and this much LDS per workgroup (csrc/intertp.hip)


def intertp_batched_fits(n_ch, Lw, max_lag):
    """Whether the batched launch takes the problem -- the launcher's own rule (bpmf_intertemplate_cc_dev): at most 63
    lags, and ONE channel of a template (Lw samples), its CCs against a tile of 8 templates (8 * n_lag) and the tile's
    weighted maxima (8 * n_ch) within the LDS budget."""
    n_lag = 2 * int(max_lag) + 1
    return max_lag <= INTERTP_MAX_LAG and 4 * (Lw + 8 * n_lag + 8 * n_ch) <= INTERTP_LDS_BYTES


def intertemplate_cc(waveforms_arr, weights, max_lag=10, device=None, pair_mask=None, symmetrise=True):
    """Pair-wise template similarity: intertp[t, u] = sum_{s,c} w[t][u,s,c] * max_lag CC, symmetrised
    (symmetrise=False: the matrix before (x + x.T) / 2).

    waveforms_arr (T,S,C,L).  weights: (T, S, C) with pair_mask (T, T) -- row t's channel weights and
    the pairs within the distance threshold, the factors the reference multiplies together
    (dataset.py:4789-4816; pair_mask may be the uint8 / bool GPU tensor of template_pair_masks, read where it lies) -- or the full (T, T, S, C) array / a callable t -> (T, S, C).  Factorised
    weights (given, or recognised in a full array) run as ONE batched launch
    (bpmf_intertemplate_cc_dev); anything else -- weights that do not factorise, more than 63 lags, a channel too long
    for the kernel's LDS budget (intertp_batched_fits, decided here before anything is launched) -- takes the
    per-template loop of the reference (intertemplate_cc_loop).  Both give the same bits."""
    import torch
    if np.shape(waveforms_arr)[-1] <= 2 * int(max_lag) or max_lag < 0:
        raise ValueError("intertemplate_cc: the waveforms must be longer than 2 * max_lag samples")
    shape = np.shape(waveforms_arr)
    if not callable(weights) and intertp_batched_fits(shape[1] * shape[2], shape[3], max_lag):
        w = np.asarray(weights, dtype=np.float32)
        fact = None
        d_mask = None
        if w.ndim == 3 and isinstance(pair_mask, torch.Tensor):      # a device mask (template_pair_masks), as it is
            d_mask = _device_pair_mask("intertemplate_cc", "pair_mask", pair_mask)
            if d_mask.shape[0] != w.shape[0]:
                raise ValueError(f"intertemplate_cc: pair_mask must be ({w.shape[0]}, {w.shape[0]})")
            fact = (w, None)
        elif w.ndim == 3:
            T = w.shape[0]
            fact = (w, np.ones((T, T), bool) if pair_mask is None else np.asarray(pair_mask, dtype=bool))
        elif w.ndim == 4 and pair_mask is None:
            fact = factorise_pair_weights(w)
        if fact is not None:
            base, mask = fact
            mf = MatchedFilterGPU(device=d_mask.device.index if d_mask is not None and device is None else device)
            wf = mf._dev(np.ascontiguousarray(waveforms_arr, dtype=np.float32), torch.float32)
            T, S, Cc, Lw = wf.shape
            base_d = mf._dev(np.ascontiguousarray(base, dtype=np.float32), torch.float32)
            if d_mask is not None:
                if d_mask.device != wf.device:
                    raise ValueError(f"intertemplate_cc: pair_mask lies on {d_mask.device}, not on {wf.device}")
                mask_d = d_mask
            else:
                mask_d = torch.as_tensor(np.ascontiguousarray(mask, dtype=np.uint8), device=wf.device)
            ws = torch.empty(mf.lib.bpmf_intertemplate_workspace_bytes(T, S, Cc, max_lag), dtype=torch.uint8,
                             device=wf.device)
            out = torch.empty((T, T), dtype=torch.float32, device=wf.device)
            from . import _lib
            _lib.call("bpmf_intertemplate_cc_dev", wf.device, wf, base_d, mask_d, T, S, Cc, Lw, int(max_lag), ws,
                      ws.numel(), _lib.STREAM, out)
            o = out.cpu().numpy()
            return (o + o.T) / 2.0 if symmetrise else o
    if isinstance(pair_mask, torch.Tensor):                  # (the loop below is driven from the host)
        pair_mask = pair_mask.cpu().numpy()
    if not callable(weights) and np.ndim(weights) == 3:     # factorised weights the batched kernel does not take
        w = np.asarray(weights, dtype=np.float32)
        T = w.shape[0]
        mask = np.ones((T, T), bool) if pair_mask is None else np.asarray(pair_mask, dtype=bool)
        weights = lambda t: w[t][None, :, :] * mask[t][:, None, None]
    return intertemplate_cc_loop(waveforms_arr, weights, max_lag=max_lag, device=device, symmetrise=symmetrise)


def intertemplate_cc_loop(waveforms_arr, weights, max_lag=10, device=None, symmetrise=True):
    """Pair-wise template similarity: intertp[t, u] = sum_{s,c} w[t][u,s,c] * max_lag CC, symmetrised
    (symmetrise=False: the matrix before (x + x.T) / 2).

    waveforms_arr (T,S,C,L); weights (T, T, S, C), or a callable t -> (T, S, C) -- row t holds the
    channel weights the reference builds for template t against every other template
    (dataset.py:4789-4816).  For each t the template's own waveform is the "data" and every
    template trimmed by max_lag on both sides is correlated against it at 2*max_lag+1 lags
    (network_sum=False, dataset.py:4818-4827).  Everything stays on the device -- the CCs, their
    max over the lags and the weighted channel sum (in numpy's summation order) -- and only the
    (T, T) matrix comes back."""
    import torch
    wf = np.ascontiguousarray(waveforms_arr, dtype=np.float32)
    if wf.shape[-1] <= 2 * int(max_lag) or max_lag < 0:
        raise ValueError("intertemplate_cc: the waveforms must be longer than 2 * max_lag samples")
    T, S, Cc = wf.shape[:3]
    mf = MatchedFilterGPU(device=device)
    wf_dev = mf._dev(wf, torch.float32)
    tp_dev = wf_dev[..., max_lag:wf.shape[-1] - max_lag].contiguous()
    mv0 = torch.zeros((T, S, Cc), dtype=torch.int32, device=wf_dev.device)
    out_dev = torch.zeros((T, T), dtype=torch.float32, device=wf_dev.device)
    for t in range(T):
        w = np.asarray(weights(t) if callable(weights) else weights[t], dtype=np.float32)
        keep = np.flatnonzero((w != 0).reshape(T, -1).sum(axis=1) > 0)
        if keep.size == 0:
            continue
        keep_dev = torch.as_tensor(keep, device=wf_dev.device)
        w_dev = mf._dev(w[keep], torch.float32)
        mf.set_data(wf_dev[t])
        cc = mf.run(tp_dev[keep_dev], mv0[keep_dev], w_dev, 1, network_sum=False)  # (n_keep, 2*max_lag+1, S, C)
        best = cc.max(dim=1).values
        out_dev[t, keep_dev] = numpy_order_sum((w_dev * best).reshape(keep.size, S * Cc))
    out = out_dev.cpu().numpy()
    return (out + out.T) / 2.0 if symmetrise else out
