#!/usr/bin/env python3
"""Generate tests/golden/multiband.npz from the REAL reference (BPMF/spectrum.py: Spectrum.compute_multi_band_spectrum
:387-505, compute_signal_to_noise_ratio :601-648) and SciPy; runs only where the reference tree and SciPy are
(make_goldens.py:import_reference).

obspy is NOT needed: the reference runs on duck-typed traces that carry .data, .id, .stats.station / .sampling_rate /
.npts and .copy(), and whose detrend / taper / filter are the three SciPy statements that obspy's documentation gives
for them (DuckTrace below).  What the file pins is therefore the reference's own logic around these three operations;
the operations themselves are settled by tools/diff_obspy_multiband.py next to a real obspy.

Only recorded results are stored; the inputs are regenerated from their seeds by tests/multiband_cases.py:

* `spectrum_f64_<k>` (E, S, C, B), `multi_f64_<k>` (E, S, B): the reference on float64 copies of the float32 windows of
  CASES[k], multi_component_spectrum False and True -- this pins the logic tightly;
* `spectrum_f32_<k>`, `multi_f32_<k>`: the reference on the float32 windows themselves -- this shows the float32
  detrend of the reference;
* `freq_<k>` (B,) float32;
* a row that holds a NaN is NOT handed to the reference (scipy.signal.detrend refuses it with a ValueError, and so does
  obspy): its recorded values are NaN, which is the definition's answer;
* `snr`, `snr_multi`: compute_signal_to_noise_ratio of SNR_CASE against noise windows that are its own events in
  another order (so that 0 / 0, x / 0 and NaN occur), the noise traces of one station of one event missing;
* `limit` = 8 x the worst deviation of postprocess.multiband_spectrum_host from the float64 run, `limit_f32` = 4 x the
  worst from the float32 run, both in the measure of multiband_cases.deviation; beyond 1e-9 / 1e-4 the restatement is
  wrong, not imprecise, and the maker stops.

Usage: python tests/golden/make_multiband_golden.py
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "multiband.npz")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SNR_CASE = 3
SNR_NOISE_EVENTS = [1, 1, 2, 4, 3]          # the event whose windows serve as the noise of event e
SNR_MISSING = (4, 2)                        # (event, station): no noise traces


class Stats:
    def __init__(self, station, sampling_rate, npts):
        self.station, self.sampling_rate, self.npts = station, sampling_rate, npts


class DuckTrace:
    """What compute_multi_band_spectrum touches of an obspy.Trace; the three operations as obspy documents them."""

    def __init__(self, data, station, channel, sampling_rate):
        self.data = data
        self.id = f"XX.{station}..{channel}"
        self.stats = Stats(station, sampling_rate, len(data))

    def copy(self):
        station, channel = self.id.split(".")[1], self.id.split(".")[3]
        return DuckTrace(self.data.copy(), station, channel, self.stats.sampling_rate)

    def detrend(self, type):
        from scipy.signal import detrend
        self.data = detrend(self.data, type=type)
        return self

    def taper(self, max_percentage, max_length=None, type="cosine"):
        assert type == "cosine"
        npts = self.stats.npts
        wlen = min(int(max_percentage * npts), int(max_length * self.stats.sampling_rate))
        assert 2 * wlen != npts
        window = np.ones(npts)
        if wlen:
            side = 0.5 * (1.0 - np.cos(np.pi * np.arange(wlen) / wlen))
            window[:wlen], window[npts - wlen:] = side, side[::-1]
        self.data = self.data * window
        return self

    def filter(self, type, freqmin, freqmax, corners, zerophase):
        from scipy.signal import iirfilter, sosfilt, zpk2sos
        assert type == "bandpass" and zerophase
        fe = 0.5 * self.stats.sampling_rate
        low, high = freqmin / fe, freqmax / fe
        assert high - 1.0 <= -1e-6                      # (obspy: a high-pass instead)
        sos = zpk2sos(*iirfilter(corners, [low, high], btype="band", ftype="butter", output="zpk"))
        first = sosfilt(sos, self.data)
        self.data = sosfilt(sos, first[::-1])[::-1]
        return self


class Distances:
    loc = type("Loc", (), {"__getitem__": lambda self, key: 10.0})()


class DuckEvent:
    hmax_unc, vmax_unc, source_receiver_dist = 1.0, 1.0, Distances()


def traces_of(x_event, sr, skip_station=None):
    S, C, _ = x_event.shape
    return [DuckTrace(x_event[s, c].copy(), f"ST{s:02d}", f"HH{c}", sr) for s in range(S) for c in range(C)
            if s != skip_station and not np.isnan(x_event[s, c]).any()]


def reference_event(Spectrum, x_event, phase, bands, sr, buffer_seconds, corners, multi, skip_station=None):
    """A Spectrum object on which compute_multi_band_spectrum has run for one event's (S, C, n) windows."""
    spec = Spectrum(event=DuckEvent())
    spec.set_frequency_bands(dict(bands))
    assert list(spec.frequency_bands) == list(bands)                  # (already in the order of the centres)
    with np.errstate(all="ignore"):
        spec.compute_multi_band_spectrum(traces_of(x_event, sr, skip_station), phase, buffer_seconds,
                                         multi_component_spectrum=multi, corners=corners)
    return spec


def as_array(table, S, C, B, multi, key="spectrum"):
    out = np.zeros((S, B) if multi else (S, C, B))
    for s in range(S):
        if multi:
            if f"ST{s:02d}" in table:
                out[s] = table[f"ST{s:02d}"][key]
        else:
            for c in range(C):
                if f"XX.ST{s:02d}..HH{c}" in table:
                    out[s, c] = table[f"XX.ST{s:02d}..HH{c}"][key]
    return out


def reference_case(Spectrum, x, bands, sr, buffer_seconds, corners, multi):
    E, S, C, _ = x.shape
    out, freq = [], None
    for e in range(E):
        spec = reference_event(Spectrum, x[e], "p", bands, sr, buffer_seconds, corners, multi)
        out.append(as_array(spec.p_spectrum, S, C, len(bands), multi))
        freq = next(iter(spec.p_spectrum.values()))["freq"]
    out = np.stack(out)
    nan_rows = np.isnan(x).any(axis=-1)                               # (the definition's answer, not the reference's)
    live = np.array([hi < sr / 2.0 for _, hi in bands.values()])       # (a skipped band stays 0)
    out[np.ix_(*[np.arange(d) for d in out.shape[:-1]], np.flatnonzero(live))] = np.where(
        (nan_rows.any(axis=-1) if multi else nan_rows)[..., None], np.nan, out[..., live])
    return out, freq


def main():
    import multiband_cases as mc
    from seismic_bpmf_amd import postprocess as pp
    spec = importlib.util.spec_from_file_location("make_goldens", os.path.join(HERE, "make_goldens.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    mg.import_reference()
    from BPMF.spectrum import Spectrum
    sr = mc.SAMPLING_RATE
    out, worst, worst_f32 = {}, 0.0, 0.0
    for k, (label, n, buffer_seconds, corners, band_key, _) in enumerate(mc.CASES):
        x, bands = mc.windows(k), mc.BANDS[band_key]
        plan = pp.multiband_plan(n, bands, sr, buffer_seconds, corners)
        prepared = pp.multiband_prepare_host(x.reshape(-1, n), plan["taper"]).reshape(x.shape)
        line = [label]
        for multi in (False, True):
            mine, freq = pp.multiband_spectrum_host(x, bands, sr=sr, buffer_seconds=buffer_seconds, corners=corners,
                                                    multi_component=multi)
            scale = mc.row_scale(x.reshape(x.shape[:2] + (-1,)), prepared.reshape(x.shape[:2] + (-1,))) if multi \
                else mc.row_scale(x, prepared)
            for tag, data in (("f64", x.astype(np.float64)), ("f32", x)):
                ref, ref_freq = reference_case(Spectrum, data, bands, sr, buffer_seconds, corners, multi)
                assert ref_freq.dtype == np.float32 and np.array_equal(ref_freq, freq), label
                dev = mc.deviation(mine, ref, scale, bands)
                line.append(f"{'multi' if multi else 'single'} {tag} {dev:.2e}")
                if tag == "f64":
                    worst = max(worst, dev)
                else:
                    worst_f32 = max(worst_f32, dev)
                out[f"{'multi' if multi else 'spectrum'}_{tag}_{k}"] = ref
            out[f"freq_{k}"] = freq
        print(", ".join(line))
    assert 8 * worst < 1e-9 and 4 * worst_f32 < 1e-4, (worst, worst_f32)    # beyond that the restatement is wrong
    out["limit"], out["limit_f32"] = np.float64(8 * worst), np.float64(4 * worst_f32)

    _, n, buffer_seconds, corners, band_key, (E, S, C) = mc.CASES[SNR_CASE]
    x, bands = mc.windows(SNR_CASE).astype(np.float64), mc.BANDS[band_key]
    for multi in (False, True):
        rows = []
        for e in range(E):
            spec = reference_event(Spectrum, x[e], "p", bands, sr, buffer_seconds, corners, multi)
            noise = reference_event(Spectrum, x[SNR_NOISE_EVENTS[e]], "noise", bands, sr, buffer_seconds, corners,
                                    multi, skip_station=SNR_MISSING[1] if e == SNR_MISSING[0] else None)
            spec.noise_spectrum = noise.noise_spectrum
            spec.phases.append("noise")
            with np.errstate(all="ignore"):
                spec.compute_signal_to_noise_ratio("p")
            rows.append(as_array(spec.snr_p_spectrum, S, C, len(bands), multi, key="snr"))
        out["snr_multi" if multi else "snr"] = np.stack(rows)
    np.savez_compressed(OUT, **out)
    print(f"limit {out['limit']:.3e}, limit_f32 {out['limit_f32']:.3e}")
    print(f"{OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
