#!/usr/bin/env python3
"""Generate tests/golden/templates.npz from the REAL reference (BPMF/dataset.py, BPMF/utils.py); runs only where the
reference tree is (make_goldens.py:import_reference).

The reference's methods are called unbound on stand-in objects that carry what they read; only arrays are stored --
the inputs of every case and what the reference made of them:

* utils.get_np_array (BPMF/utils.py:1589-1660) on a stand-in stream whose traces are what a reader hands back for the
  windows of Event.read_waveforms(time_shifted=True): the samples of [pick, pick + duration) that exist.  Full
  windows, windows cut by the END of the day (the reference pads them with zeros, :1653-1657) and windows wholly past
  it (no trace: the channel stays zero) -- `waveforms`;
* Event.set_availability (BPMF/dataset.py:2556-2607) on the same traces -- `available`;
* Family.normalize("rms" / "max") (:4152-4166) on the stacked windows -- `templates_rms`, `templates_max`;
* Template.moveouts_win / Template.moveouts_arr (:3451-3475) on a moveout table in seconds -- `moveouts_arr`;
* the noise windows of Event.compute_snr (time_shifted=False: one start for every channel) through get_np_array again,
  and then the two np.std lines of compute_snr themselves (:1457-1461) -- `snr`.  compute_snr as a whole cannot be
  driven without obspy (it deep-copies the event and reads through Event.read_waveforms, which builds an
  obspy.Stream, :1997-2052): those lines are pinned through NumPy alone, on the arrays the reference's get_np_array
  returned.

Windows cut by the START of the day are not in this file: there the package departs from the reference on purpose
(postprocess.templates_from_events_host).

Usage: python tests/golden/make_templates_golden.py
"""
import importlib.util
import os
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "templates.npz")
STATIONS = ["STA1", "STA2", "STA3", "STA4"]
COMPONENTS = ["N", "E", "Z"]
ALIASES = {"N": ["N", "1"], "E": ["E", "2"], "Z": ["Z"]}
PHASES = ["P", "S"]
PHASE_ON_COMP = {"N": "S", "1": "S", "E": "S", "2": "S", "Z": "P"}


class Trace:
    def __init__(self, station, channel, data):
        self.station, self.channel, self.component, self.data = station, channel, channel[-1], data


class Stream(list):
    """What the reference asks of an obspy.Stream: select(station=, component=, channel=) and indexing."""

    def select(self, station=None, component=None, channel=None):
        return Stream(tr for tr in self if (station is None or tr.station == station) and
                      (component is None or tr.component == component) and (channel is None or tr.channel == channel))


def day(rng, n):
    """(S, C, n) float32: noise, an all-zero channel, a constant one, one holding a NaN, one of tiny amplitudes."""
    data = rng.standard_normal((len(STATIONS), len(COMPONENTS), n)).astype(np.float32)
    data[1, 0] = 0.0
    data[1, 2] = np.float32(-2.5)
    data[2, 1, n // 3::97] = np.nan
    data[3, 0] *= np.float32(1e-20)
    data[3, 1, ::3] = -0.0
    return data


def read_windows(data, start, n_samples):
    """The traces a reader returns for the windows [start[s, c], + n_samples) of the day: the samples that exist.
    Station 3 names its horizontal components 1 and 2, station 4 its channels BH*."""
    stream = Stream()
    n = data.shape[-1]
    for s, sta in enumerate(STATIONS):
        for c, cp in enumerate(COMPONENTS):
            a, b = int(start[s, c]), min(int(start[s, c]) + n_samples, n)
            assert a >= 0
            if b <= a:
                continue
            name = {"N": "1", "E": "2"}.get(cp, cp) if s == 2 else cp
            stream.append(Trace(sta, ("BH" if s == 3 else "HH") + name, data[s, c, a:b].copy()))
    return stream


def reference_case(BPMF, rng, n, n_samples, sr, n_events, noise_offset, noise_samples):
    import pandas as pd
    from BPMF import dataset, utils
    data = day(rng, n)
    S, C = data.shape[:2]
    moveouts_sec = rng.uniform(0.0, 12.0, (n_events, S, len(PHASES)))
    moveouts_sec[..., 1] += moveouts_sec[..., 0]                     # S after P
    moveouts_sec[-2:, 0, 0] = 0.5                                    # (the late events keep at least one trace)
    offset_sec = np.array([1.0, 4.0])
    phase_of_component = np.array([PHASES.index(PHASE_ON_COMP[cp]) for cp in COMPONENTS])
    # origins: inside the day, the last two so late that their windows are cut by the end of the day / lie past it
    origin = rng.integers(max(int(5 * sr), noise_offset), n - n_samples - int(30 * sr), n_events).astype(np.int64)
    origin[-2] = n - n_samples
    origin[-1] = n - int(3 * sr)
    mv_arr = np.zeros((n_events, S, C), dtype=np.int32)
    waveforms = np.zeros((n_events, S, C, n_samples), dtype=np.float32)
    noise = np.zeros((n_events, S, C, noise_samples), dtype=np.float32)
    available = np.zeros((n_events, S, C), dtype=bool)
    for e in range(n_events):
        aux = {f"offset_{ph}": offset_sec[p] for p, ph in enumerate(PHASES)}
        aux.update({f"phase_on_comp{cp}": ph for cp, ph in PHASE_ON_COMP.items()})
        tp = types.SimpleNamespace(
            moveouts=pd.DataFrame(moveouts_sec[e], index=STATIONS, columns=[f"moveouts_{ph}" for ph in PHASES]),
            phases=PHASES, aux_data=aux, stations=STATIONS, components=COMPONENTS, sr=sr)
        tp.moveouts_win = dataset.Template.moveouts_win.fget(tp)
        mv_arr[e] = dataset.Template.moveouts_arr.fget(tp)
        assert mv_arr[e].min() + origin[e] >= 0
        tp.traces = read_windows(data, origin[e] + mv_arr[e], n_samples)
        assert len(tp.traces) > 0                                    # (get_np_array returns None for an empty stream)
        tp.set_aux_data = lambda d: None
        waveforms[e] = utils.get_np_array(tp.traces, STATIONS, components=COMPONENTS, priority="HH",
                                          component_aliases=ALIASES, n_samples=n_samples, verbose=False)
        dataset.Event.set_availability(tp, components=COMPONENTS, component_aliases=ALIASES)
        available[e] = tp._availability_per_cha[COMPONENTS].values
        start = np.full((S, C), origin[e] - noise_offset)
        noise[e] = utils.get_np_array(read_windows(data, start, noise_samples), STATIONS, components=COMPONENTS,
                                      priority="HH", component_aliases=ALIASES, n_samples=noise_samples, verbose=False)
    out = {"data": data, "origin": origin, "moveouts_sec": moveouts_sec, "offset_sec": offset_sec,
           "phase_of_component": phase_of_component, "sr": np.float64(sr), "n_samples": np.int64(n_samples),
           "noise_offset": np.int64(noise_offset), "noise_samples": np.int64(noise_samples), "moveouts_arr": mv_arr,
           "waveforms": waveforms, "available": available}
    with np.errstate(invalid="ignore"):
        for method in ("rms", "max"):
            arr = waveforms.copy()
            group = types.SimpleNamespace(waveforms_arr=arr, _waveforms_arr=arr, _remember=lambda name: None)
            dataset.Family.normalize(group, method=method)
            out[f"templates_{method}"] = group._waveforms_arr
        # Event.compute_snr, BPMF/dataset.py:1457-1461, on the arrays get_np_array returned
        noise_std = np.std(noise, axis=-1)
        noise_std[noise_std == 0.0] = 1.0
        signal_std = np.std(waveforms, axis=-1)
        out["snr"] = signal_std / noise_std
    assert available.any() and not available.all() and np.isnan(out["templates_rms"]).any()
    return out


def main():
    spec = importlib.util.spec_from_file_location("make_goldens", os.path.join(HERE, "make_goldens.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    BPMF, _ = mg.import_reference()
    rng = np.random.default_rng(20261018)
    cases = [reference_case(BPMF, rng, 2500, 200, 25.0, 6, 150, 125),
             reference_case(BPMF, rng, 3001, 129, 40.0, 5, 50, 257),
             reference_case(BPMF, rng, 3503, 520, 50.0, 3, 600, 500)]
    out = {"n_cases": np.int64(len(cases))}
    for j, case in enumerate(cases):
        out.update({f"{k}_{j}": v for k, v in case.items()})
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(cases)} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
