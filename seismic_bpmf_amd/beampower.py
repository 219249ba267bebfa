"""Backprojection call surface: a drop-in for ``beampower.beampower.beamform``.

The reference calls it at BPMF/template_search.py:549-558 and :560-569::

    bp.beampower.beamform(waveform_features, moveouts, weights_phases, weights_sources,
                          device=device, out_of_bounds=out_of_bounds,
                          num_threads=num_threads, reduce=reduce)

``reduce="max"`` returns ``(maxbeam float32[N], argmax int32[N])``; ``reduce="none"`` returns
``beam float32[K, N]``.  Work runs on the MI355X through libbpmf_hip.so; ``device="cpu"``
raises (no CPU path in this package).

:class:`BeamformerGPU` is the device-resident form: the moveout table / source weights are
planned and uploaded once (the reference rebuilds its table on every access,
template_search.py:444-454) and then reused for every day of features.
"""
import ctypes as C

import numpy as np

from . import _lib

GPU_DEVICES = ("gpu", "hip", "mi355x")
_OOB = {"strict": 0, "flexible": 1}
_REDUCE = {"max": 0, "none": 1}


def _check_shapes(features, moveouts, w_phases, w_sources):
    f = np.ascontiguousarray(features, dtype=np.float32)
    if f.ndim != 3:
        raise ValueError("waveform_features must be (n_stations, n_components, n_samples)")
    S, Cc, N = f.shape
    mv = np.ascontiguousarray(moveouts, dtype=np.int32)  # delivered as int64 by BPMF (utils.py:1270)
    if mv.ndim != 3 or mv.shape[1] != S:
        raise ValueError("moveouts must be (n_sources, n_stations, n_phases)")
    K, _, P = mv.shape
    wp = np.ascontiguousarray(w_phases, dtype=np.float32)
    if wp.shape != (S, Cc, P):
        raise ValueError(f"weights_phases must be ({S}, {Cc}, {P}); got {wp.shape}")
    ws = np.ascontiguousarray(w_sources, dtype=np.float32)
    if ws.shape != (K, S):
        raise ValueError(f"weights_sources must be ({K}, {S}); got {ws.shape}")
    return f, mv, wp, ws


def beamform(waveform_features, time_delays, weights_phases, weights_sources, device="gpu",
             reduce="max", mode="direct", out_of_bounds="strict", num_threads=None,
             device_id=None):
    """Shift-and-stack beam power over a grid of sources (see module docstring).

    ``device_id``: None (default) = all visible GPUs, the source grid block-partitioned among them
    inside the library (``bpmf_bp_run_multi``: one host thread per GPU) and, for ``reduce="max"``,
    the per-GPU maxima merged in block order with a strict ``>`` -- blocks hold ascending source
    indices, so ties keep the lowest index exactly like a single pass; an int or a list selects
    devices."""
    del num_threads  # CPU-only knob of the reference; accepted for call compatibility
    from .matched_filter import require_gpu_arch
    require_gpu_arch(device, "device")
    if mode != "direct":
        raise NotImplementedError("only mode='direct' is implemented")
    if reduce not in _REDUCE:
        raise ValueError("reduce should be 'max' or 'none'")
    if out_of_bounds not in _OOB:
        raise ValueError("out_of_bounds should be 'strict' or 'flexible'")
    from .matched_filter import _device_array, _device_list
    f, mv, wp, ws = _check_shapes(waveform_features, time_delays, weights_phases, weights_sources)
    S, Cc, N = f.shape
    K, _, P = mv.shape
    pf, pi = _lib._f, _lib._i
    lib = _lib.lib()
    n_dev, dev_arr = _device_array(_device_list(device_id))
    if reduce == "none":
        beam = np.empty((K, N), dtype=np.float32)
        arg = None
    else:
        beam = np.empty(N, dtype=np.float32)
        arg = np.empty(N, dtype=np.int32)
    rc = lib.bpmf_bp_run_multi(f.ctypes.data_as(pf), mv.ctypes.data_as(pi), wp.ctypes.data_as(pf),
                               ws.ctypes.data_as(pf), N, K, S, Cc, P, _OOB[out_of_bounds],
                               _REDUCE[reduce], n_dev, dev_arr, beam.ctypes.data_as(pf),
                               arg.ctypes.data_as(pi) if arg is not None else None)
    _lib.check(rc, "bpmf_bp_run_multi")
    return beam if reduce == "none" else (beam, arg)


def source_coordinate_tables(longitude, latitude, depth, K):
    """The (6, K) float64 tables of bpmf_bp_location_uncertainty_dev from the coordinates of K source rows:
    longitude, latitude, depth, postprocess.domain_scale_per_latitude, sin and cos of the reduced latitude.
    Wrong lengths and values that are not finite raise ValueError (host only: no device is touched)."""
    from . import postprocess as pp
    cols = []
    for name, x in (("longitude", longitude), ("latitude", latitude), ("depth", depth)):
        x = np.asarray(x, dtype=np.float64)
        if x.shape != (K,):
            raise ValueError(f"{name} must be ({K},), one value per source row of the plan; got {x.shape}")
        if not np.isfinite(x).all():
            raise ValueError(f"{name} holds values that are not finite")
        cols.append(x)
    if np.abs(cols[1]).max(initial=0.0) > 90.0:
        raise ValueError("latitude outside [-90, 90] degrees")
    su, cu = pp.reduced_latitude_sin_cos(cols[1])
    return np.ascontiguousarray(np.stack(cols + [pp.domain_scale_per_latitude(cols[1]), su, cu]))


class BeamformerGPU:
    """Device-resident beamformer bound to one moveout table and one set of source weights."""
    _coord_tables = None         # set_source_coordinates
    source_coordinates = None

    def __init__(self, moveouts, weights_sources, device=None, source_id_offset=0):
        import torch
        self.torch = torch
        if not torch.cuda.is_available():
            raise _lib.BpmfHipError("BeamformerGPU needs a HIP device")
        idx = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", idx)
        self.lib = _lib.lib()
        mv = np.ascontiguousarray(moveouts, dtype=np.int32)
        ws = np.ascontiguousarray(weights_sources, dtype=np.float32)
        if mv.ndim != 3 or ws.shape != mv.shape[:2]:
            raise ValueError("moveouts must be (K, S, P) and weights_sources (K, S)")
        self.K, self.S, self.P = mv.shape
        self.source_id_offset = int(source_id_offset)
        self._tables_host = (mv, ws)     # relocate_batch gathers beam columns from the tables as they are
        self._tables_dev = None
        self._plan = _lib.Handle()
        rc = self.lib.bpmf_bp_plan_create(mv.ctypes.data_as(_lib._i), ws.ctypes.data_as(_lib._f),
                                          self.K, self.S, self.P, idx, int(source_id_offset),
                                          C.byref(self._plan))
        _lib.check(rc, "bpmf_bp_plan_create")
        self._ws = None

    def plan_info(self):
        """Shape of the device plan: dict of bpmf_bp_plan_stats (include/bpmf_hip.h)."""
        st = _lib.BpPlanStats()
        _lib.check(self.lib.bpmf_bp_plan_info(self._plan, C.byref(st)), "bpmf_bp_plan_info")
        out = {}
        for n, _ in st._fields_:
            v = getattr(st, n)
            out[n] = int(v) if isinstance(v, int) else [int(x) for x in v]
        return out

    def close(self):
        if getattr(self, "_plan", None) is not None and self._plan.value:
            self.lib.bpmf_bp_plan_destroy(self._plan)
            self._plan = _lib.Handle()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _dev(self, arr, dtype):
        t = self.torch
        if isinstance(arr, t.Tensor):
            return arr.to(device=self.device, dtype=dtype).contiguous()
        return t.as_tensor(np.ascontiguousarray(arr), dtype=dtype, device=self.device).contiguous()

    def run(self, features, weights_phases, reduce="max", out_of_bounds="strict", out=None):
        """Beamform one (S, C, N) feature array.  Returns device tensors."""
        t = self.torch
        f = self._dev(features, t.float32)
        S, Cc, N = f.shape
        if S != self.S:
            raise ValueError("features and moveouts disagree on the number of stations")
        wp = self._dev(weights_phases, t.float32)
        if tuple(wp.shape) != (S, Cc, self.P):
            raise ValueError(f"weights_phases must be ({S}, {Cc}, {self.P})")
        nbytes = self.lib.bpmf_bp_workspace_bytes(self._plan, N, Cc)
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = t.empty(nbytes, dtype=t.uint8, device=self.device)
        if reduce == "max":
            beam, arg = out if out is not None else (
                t.empty(N, dtype=t.float32, device=self.device),
                t.empty(N, dtype=t.int32, device=self.device))
        else:
            beam = out if out is not None else t.empty((self.K, N), dtype=t.float32,
                                                       device=self.device)
            arg = None
        _lib.call("bpmf_bp_run_dev", self.device, self._plan, f, wp, N, Cc, _OOB[out_of_bounds], _REDUCE[reduce],
                  self._ws, self._ws.numel(), _lib.STREAM, beam, arg)
        self._keepalive = (f, wp)
        return (beam, arg) if reduce == "max" else beam

    _METHOD = {"spatial": 0, "temporal": 1}

    def relocation_workspace_bytes(self, E, N, Cc):
        return int(self.lib.bpmf_bp_relocate_workspace_bytes(self._plan, int(E), int(N), int(Cc)))

    def relocate_batch(self, features, event_stride, row_stride, starts, weights_phases, E, N, Cc,
                       out_of_bounds, method, workspace, time_idx, src_idx, max_beam, likelihood=None,
                       columns=None, maxbeam=None, maxbeam_sources=None):
        """bpmf_bp_relocate_batch_dev (include/bpmf_hip.h) on device tensors: the point of maximum focusing of E
        events in shared launches, written to the caller's output tensors.  `features` / `starts`: see the
        header for the two layouts.  workflow.relocate_events is the call with checks, chunks and results."""
        t = self.torch
        if method == "spatial" and self._tables_dev is None:
            mv, ws = self._tables_host
            self._tables_dev = (t.as_tensor(mv, device=self.device), t.as_tensor(ws, device=self.device))
        mv_d, ws_d = self._tables_dev if method == "spatial" else (None, None)
        _lib.call("bpmf_bp_relocate_batch_dev", self.device, self._plan, features, int(event_stride), int(row_stride),
                  starts, weights_phases, mv_d, ws_d, int(E), int(N), int(Cc), _OOB[out_of_bounds], self._METHOD[method],
                  workspace, workspace.numel(), _lib.STREAM, time_idx, src_idx, max_beam, likelihood, columns, maxbeam,
                  maxbeam_sources)

    def set_source_coordinates(self, longitude, latitude, depth):
        """Coordinates of this plan's source rows, three (K,) arrays: degrees, degrees, km -- what
        ``Beamformer.set_source_coordinates`` (BPMF/template_search.py:753) keeps in a DataFrame.  The float64
        tables of bpmf_bp_location_uncertainty_dev are built and uploaded once, here."""
        tables = source_coordinate_tables(longitude, latitude, depth, self.K)
        self.source_coordinates = {"longitude": tables[0].copy(), "latitude": tables[1].copy(),
                                   "depth": tables[2].copy()}
        self._coord_tables = self.torch.as_tensor(tables, device=self.device)

    def uncertainty_workspace_bytes(self, E, n_terms):
        return int(self.lib.bpmf_bp_location_uncertainty_workspace_bytes(int(E), int(n_terms)))

    def location_uncertainty(self, method, E, N, src_idx, workspace, out, n_domain, likelihood=None, maxbeam=None,
                             maxbeam_sources=None, max_beam=None, side_km=100.0, effective_kT=0.33,
                             gibbs_cutoff=0.25, domain_mask=None):
        """bpmf_bp_location_uncertainty_dev (include/bpmf_hip.h) on device tensors, behind relocate_batch on the
        same stream: `out` (5, E) float64 receives hunc, vunc, longitude, latitude, depth and `n_domain` (E,)
        int32 the size of the domain.  workflow.relocate_events(uncertainties=True) is the call with checks."""
        from . import postprocess as pp
        if getattr(self, "_coord_tables", None) is None:
            raise ValueError("no source coordinates: call set_source_coordinates(longitude, latitude, depth) first")
        _lib.call("bpmf_bp_location_uncertainty_dev", self.device, self._plan, self._METHOD[method], int(E), int(N),
                  src_idx, likelihood, maxbeam, maxbeam_sources, max_beam, self._coord_tables,
                  pp.domain_scale_per_longitude(), float(side_km) / 2.0, float(effective_kT), float(gibbs_cutoff),
                  workspace, workspace.numel(), _lib.STREAM, out[0], out[1], n_domain, out[2], out[3], out[4],
                  domain_mask)

    # -- multi-GPU exchange step of reduce="max"  ----------------
    def pack_max(self, beam, arg):
        """(beam, arg) -> int64 keys whose max is (largest beam, lowest source id)."""
        t = self.torch
        packed = t.empty(beam.numel(), dtype=t.int64, device=self.device)
        _lib.call("bpmf_bp_pack_max_dev", self.device, beam, arg, beam.numel(), 1, _lib.STREAM, packed)
        return packed

    def unpack_max(self, packed):
        t = self.torch
        n = packed.numel()
        beam = t.empty(n, dtype=t.float32, device=self.device)
        arg = t.empty(n, dtype=t.int32, device=self.device)
        _lib.call("bpmf_bp_unpack_max_dev", self.device, packed, n, 1, _lib.STREAM, beam, arg)
        return beam, arg
