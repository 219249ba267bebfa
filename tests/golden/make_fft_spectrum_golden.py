#!/usr/bin/env python3
"""Generate tests/golden/fft_spectrum.npz from the REAL reference (BPMF/spectrum.py: Spectrum.compute_spectrum :507-599,
Spectrum.resample :851-887, compute_signal_to_noise_ratio :601-648); runs only where the reference tree and SciPy are
(make_goldens.py:import_reference).

No obspy operation is involved in this method: the reference runs on duck-typed traces that carry .data, .id and
.stats.station / .sampling_rate / .npts / .delta.

Only recorded results are stored; the inputs are regenerated from their seeds by tests/fft_spectrum_cases.py.  For
every (case, dtype, alpha) of fc.RECORDED, on the float32 windows themselves ("f32") or on float64 copies ("f64"):

* `single_<case>_<dtype>_<alpha>`: compute_spectrum per component, then resample onto the case's targets:
  (E, S, C, F) float64 -- or, for a case without targets, the complex spectrum itself (E, S, C, K);
* `multi_<case>_<dtype>_<alpha>`: the same with multi_component_spectrum=True: (E, S, F) or (E, S, K) float64;
* a row that holds a NaN is handed to the reference like every other, but its recorded values are then SET to what the
  definition states (NaN wherever the reference does not zero the target), whatever the FFT made of it;
* `snr`, `snr_multi`: compute_signal_to_noise_ratio of the resampled spectra of SNR_CASE against noise windows that are
  its own events in another order (so that 0 / 0, x / 0 and NaN occur), the noise traces of one station of one event
  missing;
* `numpy_version`: the NumPy that made the file (its pocketfft and np.interp are part of what is recorded).

Usage: python tests/golden/make_fft_spectrum_golden.py
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "fft_spectrum.npz")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


class Stats:
    def __init__(self, station, sampling_rate, npts):
        self.station, self.sampling_rate, self.npts, self.delta = station, sampling_rate, npts, 1.0 / sampling_rate


class DuckTrace:
    """What compute_spectrum touches of an obspy.Trace."""

    def __init__(self, data, station, channel, sampling_rate):
        self.data = data
        self.id = f"XX.{station}..{channel}"
        self.stats = Stats(station, sampling_rate, len(data))


class Distances:
    loc = type("Loc", (), {"__getitem__": lambda self, key: 10.0})()


class DuckEvent:
    hmax_unc, vmax_unc, source_receiver_dist = 1.0, 1.0, Distances()

    def __init__(self, n, sr):
        self.duration = (n + 0.5) / sr            # int(duration * sr) == n, whatever the rounding of n / sr * sr


def reference_event(Spectrum, x_event, phase, sr, alpha, multi, frequencies, skip_station=None):
    """A Spectrum object on which compute_spectrum (and, with targets, resample) has run for one event's (S, C, n)
    windows."""
    S, C, n = x_event.shape
    traces = [DuckTrace(x_event[s, c].copy(), f"ST{s:02d}", f"HH{c}", sr) for s in range(S) for c in range(C)
              if s != skip_station]
    spec = Spectrum(event=DuckEvent(n, sr))
    with np.errstate(all="ignore"):
        spec.compute_spectrum(traces, phase, multi_component_spectrum=multi, alpha=alpha)
        if frequencies is not None:
            spec.resample(frequencies, phase)
    return spec


def as_array(table, S, C, width, multi, key="spectrum", dtype=np.float64):
    out = np.zeros((S, width) if multi else (S, C, width), dtype=dtype)
    for s in range(S):
        if multi:
            if f"ST{s:02d}" in table:
                out[s] = table[f"ST{s:02d}"][key]
        else:
            for c in range(C):
                if f"XX.ST{s:02d}..HH{c}" in table:
                    out[s, c] = table[f"XX.ST{s:02d}..HH{c}"][key]
    return out


def reference_case(Spectrum, x, sr, alpha, multi, frequencies):
    E, S, C, n = x.shape
    width = n // 2 + 1 if frequencies is None else len(frequencies)
    dtype = np.complex128 if frequencies is None and not multi else np.float64
    out = np.stack([as_array(reference_event(Spectrum, x[e], "p", sr, alpha, multi, frequencies).p_spectrum, S, C,
                             width, multi, dtype=dtype) for e in range(E)])
    nan_rows = np.isnan(x).any(axis=-1)                               # (the definition's answer, not the FFT's)
    nan_rows = nan_rows.any(axis=-1) if multi else nan_rows
    keep = np.ones(width, dtype=bool)
    if frequencies is not None:
        keep = ~(frequencies >= 0.99 * np.fft.rfftfreq(n, d=1.0 / sr).max())
    out[np.ix_(*[np.arange(d) for d in out.shape[:-1]], np.flatnonzero(keep))] = np.where(
        nan_rows[..., None], complex(np.nan, np.nan) if dtype == np.complex128 else np.nan, out[..., keep])
    return out


def main():
    import fft_spectrum_cases as fc
    spec = importlib.util.spec_from_file_location("make_goldens", os.path.join(HERE, "make_goldens.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    mg.import_reference()
    from BPMF.spectrum import Spectrum
    sr = fc.SAMPLING_RATE
    out = {}
    for index, dtype, alpha in fc.RECORDED:
        n, key, _ = fc.CASES[index]
        x = fc.windows(index).astype(np.float32 if dtype == "f32" else np.float64)
        for multi in (False, True):
            out[fc.recorded_key(index, dtype, alpha, multi)] = reference_case(Spectrum, x, sr, alpha, multi,
                                                                              fc.targets(key, n))
        print(fc.label(index), dtype, alpha)

    n, key, (E, S, C) = fc.CASES[fc.SNR_CASE]
    x, frequencies = fc.windows(fc.SNR_CASE), fc.targets(key, n)
    for multi in (False, True):
        rows = []
        for e in range(E):
            spec = reference_event(Spectrum, x[e], "p", sr, 0.05, multi, frequencies)
            noise = reference_event(Spectrum, x[fc.SNR_NOISE_EVENTS[e]], "noise", sr, 0.05, multi, frequencies,
                                    skip_station=fc.SNR_MISSING[1] if e == fc.SNR_MISSING[0] else None)
            spec.noise_spectrum = noise.noise_spectrum
            spec.phases.append("noise")
            with np.errstate(all="ignore"):
                spec.compute_signal_to_noise_ratio("p")
            rows.append(as_array(spec.snr_p_spectrum, S, C, len(frequencies), multi, key="snr"))
        out["snr_multi" if multi else "snr"] = np.stack(rows)
    out["numpy_version"] = np.array(np.__version__)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
