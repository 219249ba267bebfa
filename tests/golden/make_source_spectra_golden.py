#!/usr/bin/env python3
"""Generate tests/golden/source_spectra.npz from the REAL reference (BPMF/spectrum.py: compute_signal_to_noise_ratio
:601-648, set_Q_model :37-63, compute_correction_factor :97-198, correct_geometrical_spreading :200-227,
correct_attenuation :229-256, compute_network_average_spectrum :258-386, approximate_moment_magnitude :1341-1496);
runs only where the reference tree, SciPy and pandas are (make_goldens.py:import_reference).

The Spectrum methods run on duck-typed events: pandas Series for the distances, a DataFrame for `arrival_times`, dicts
for the spectra.  Only recorded results are stored; the inputs are regenerated from their seeds by
tests/source_spectra_cases.py.  For every case of sc.RECORDED and phase ("p", "s"), with <k> = <case>_<phase>:

* `geometry_<k>` (E, S), `att_physical_<k>`, `att_reference_<k>` (E, S, F): the factor tables after
  compute_correction_factor, and after correct_attenuation's update_attenuation_factor; NaN rows for absent stations
  do not occur (the tables hold every station of the event);
* `snr_<k>`, `corrected_<k>`: shaped as the case's spectra, 0 for an absent station;
* `avg_<k>_<o>`, `std_<k>_<o>` (E, F) float64 (NaN where masked, each by its own mask), `mask_<k>_<o>` (E, F) bool (the
  average's), `nvalid_<k>_<o>` (E, F)
  int64, `nused_<k>_<o>` (E,) (the number of spectra that entered), for option o of sc.AVERAGE_OPTIONS;
* for the cases with (E, S, F) spectra (the reference's approximate_moment_magnitude runs only with
  multi_component_spectrum=True), for option o of sc.MW_OPTIONS: `mw_<k>_<o>` (E,) float64, `msnr_<k>_<o>` and
  `rawweights_<k>_<o>` (E, S) float32: what the `snr_based_weights` callable was handed and returned (0 for an absent
  station), `mwraised_<k>_<o>` (E,) bool: the call raised (an empty selection of bands: the reference's unused argmax);
* for every case of sc.STAGE4_RECORDED (corrected spectra, SNR and epicentral distances handed to
  approximate_moment_magnitude as they are, phase "p") the same four arrays as `mw_<case>_<o>`, `msnr_<case>_<o>`,
  `rawweights_<case>_<o>`, `mwraised_<case>_<o>`; events with a NaN or inf distance are recorded as they come and are
  not compared (there the reference clips a pandas Series, which reads a NaN bound as no bound);
* `numpy_version`, `pandas_version`.

Usage: python tests/golden/make_source_spectra_golden.py
"""
import contextlib
import importlib.util
import io
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "source_spectra.npz")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


class DuckEvent:
    """What the correction, averaging and magnitude methods touch of a BPMF.dataset.Event."""

    def __init__(self, pd, names, dist, epi, tt_p, tt_s, hmax, vmax):
        self.source_receiver_dist = pd.Series(dist, index=names)
        self._source_receiver_dist = self.source_receiver_dist
        self.source_receiver_epicentral_dist = pd.Series(epi, index=names)
        self.arrival_times = pd.DataFrame({"P_tt_sec": tt_p, "S_tt_sec": tt_s}, index=names)
        self.hmax_unc, self.vmax_unc = hmax, vmax


def spectrum_ids(S, C):
    """[(spectrum id, station index, component index or None)] in the order of the channels."""
    if C == 0:
        return [(f"ST{s:02d}", s, None) for s in range(S)]
    return [(f"XX.ST{s:02d}..HH{c}", s, c) for s in range(S) for c in range(C)]


def reference_event(pd, Spectrum, sc, x, e, phase, signal):
    S = x["present"].shape[1]
    C = 0 if signal.ndim == 3 else signal.shape[2]
    names = [f"ST{s:02d}" for s in range(S)]
    event = DuckEvent(pd, names, x["dist"][e], x["epi"][e], x["tt_p"][e], x["tt_s"][e], x["hmax"][e], x["vmax"][e])
    spec = Spectrum(event=event)
    spec.frequencies = np.array(x["frequencies"])
    spec.phases = ["noise", phase]
    spec.multi_component_spectrum = C == 0
    table, noise = {}, {}
    max_err = np.sqrt(event.hmax_unc ** 2 + event.vmax_unc ** 2)                    # as compute_spectrum :439-442
    for sid, s, c in spectrum_ids(S, C):
        index = (e, s) if c is None else (e, s, c)
        if x["present"][e, s]:
            table[sid] = {"spectrum": np.array(signal[index]), "freq": spec.frequencies,
                          "relative_distance_err_pct": 100.0 * (max_err / event.source_receiver_dist.loc[names[s]])}
        if x["noise_present"][e, s]:
            noise[sid] = {"spectrum": np.array(x["noise"][index]), "freq": spec.frequencies}
    setattr(spec, f"{phase}_spectrum", table)
    spec.noise_spectrum = noise
    return spec


def gather(table, S, C, F, key, dtype=np.float64):
    out = np.zeros((S, F) if C == 0 else (S, C, F), dtype=dtype)
    for sid, s, c in spectrum_ids(S, C):
        if sid in table:
            out[s if c is None else (s, c)] = table[sid][key]
    return out


def main():
    import pandas as pd
    import source_spectra_cases as sc
    spec_ = importlib.util.spec_from_file_location("make_goldens", os.path.join(HERE, "make_goldens.py"))
    mg = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(mg)
    mg.import_reference()
    from BPMF.spectrum import Spectrum, approximate_moment_magnitude, _snr_based_weights
    warnings.simplefilter("ignore")
    m = sc.MEDIUM
    out = {}
    for name in sc.RECORDED:
        x = sc.inputs(name)
        E, S = x["present"].shape
        F = len(x["frequencies"])
        for phase in sc.PHASES:
            k = f"{name}_{phase}"
            signal = sc.phase_arguments(name, phase)["signal"]
            C = 0 if signal.ndim == 3 else signal.shape[2]
            rows = {}

            def put(key, e, value):
                rows.setdefault(key, [None] * E)[e] = value

            for e in range(E):
                spec = reference_event(pd, Spectrum, sc, x, e, phase, signal)
                with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
                    spec.compute_signal_to_noise_ratio(phase)
                    Q = m["Q_1HZ"] * np.power(spec.frequencies, m["attenuation_n"])
                    spec.set_Q_model(Q, spec.frequencies, Q_phase_prefactor=sc.PREFACTOR)
                    spec.compute_correction_factor(m["rho_source_kgm3"], m["rho_receiver_kgm3"], m["vp_source_ms"],
                                                   m["vp_receiver_ms"], m["vs_source_ms"], m["vs_receiver_ms"])
                    names = [f"ST{s:02d}" for s in range(S)]
                    column = f"attenuation_{phase.upper()}"
                    put(f"geometry_{k}", e, np.array([spec.geometrical_factor.loc[n, f"geometry_{phase.upper()}"]
                                                      for n in names], dtype=np.float64))
                    put(f"att_physical_{k}", e, np.stack([np.asarray(spec.attenuation_factor.loc[n, column],
                                                                     dtype=np.float64) for n in names]))
                    spec.correct_geometrical_spreading()
                    spec.correct_attenuation()
                    put(f"att_reference_{k}", e, np.stack([np.asarray(spec.attenuation_factor.loc[n, column],
                                                                      dtype=np.float64) for n in names]))
                    put(f"snr_{k}", e, gather(getattr(spec, f"snr_{phase}_spectrum"), S, C, F, "snr"))
                    put(f"corrected_{k}", e, gather(getattr(spec, f"{phase}_spectrum"), S, C, F, "spectrum"))
                    for o, option in enumerate(sc.AVERAGE_OPTIONS):
                        for attribute in ("average_spectra", f"average_{phase}_spectrum"):
                            if hasattr(spec, attribute):
                                delattr(spec, attribute)
                        spec.compute_network_average_spectrum(
                            phase, sc.THRESHOLD, average_log=option[0], reduce=option[1],
                            min_num_valid_channels_per_freq_bin=option[2], max_relative_distance_err_pct=option[3])
                        if spec.average_spectra == []:
                            avg, std = np.full(F, np.nan), np.full(F, np.nan)
                            mask, nvalid, nused = np.ones(F, bool), np.zeros(F, np.int64), 0
                        else:
                            result = getattr(spec, f"average_{phase}_spectrum")
                            mask = np.ma.getmaskarray(result["spectrum"]) | np.zeros(F, bool)
                            avg = np.where(mask, np.nan, np.ma.getdata(result["spectrum"]))
                            std = np.where(np.ma.getmaskarray(result["std"]) | np.zeros(F, bool), np.nan,
                                           np.ma.getdata(result["std"]) + np.zeros(F))
                            nvalid, nused = np.asarray(result["num_valid_channels"]), len(result["spectra"])
                        for key, value in (("avg", avg), ("std", std), ("mask", mask), ("nvalid", nvalid),
                                           ("nused", nused)):
                            put(f"{key}_{k}_{o}", e, value)
                    if C != 0:
                        continue
                    present = np.flatnonzero(x["present"][e])
                    for o, option in enumerate(sc.MW_OPTIONS):
                        seen = {}

                        def capture(snr, snr_threshold, **kw):
                            seen["snr"] = snr.copy()
                            seen["weights"] = _snr_based_weights(snr, snr_threshold, **kw).copy()
                            return seen["weights"].copy()

                        msnr, raw = np.zeros(S, np.float32), np.zeros(S, np.float32)
                        try:
                            value = approximate_moment_magnitude(
                                spec, snr_threshold=sc.THRESHOLD, num_averaging_bands=option[0],
                                low_snr_freq_min_hz=option[1], magnitude_log_moment_scaling=sc.SCALING,
                                phases=[phase], snr_based_weights=capture)[phase]
                            msnr[present], raw[present] = seen["snr"], seen["weights"]
                            raised = False
                        except ValueError:
                            value, raised = np.nan, True
                        for key, v in (("mw", value), ("msnr", msnr), ("rawweights", raw), ("mwraised", raised)):
                            put(f"{key}_{k}_{o}", e, v)
            for key, values in rows.items():
                out[key] = np.stack([np.asarray(v) for v in values])
            print(k)
    # the stage-4 cases: corrected spectra, SNR and distances handed to approximate_moment_magnitude as they are
    for name in sc.STAGE4_RECORDED:
        x = sc.stage4_inputs(name)
        E, S = x["present"].shape
        names = [f"ST{s:02d}" for s in range(S)]
        rows = {}
        for e in range(E):
            event = DuckEvent(pd, names, x["epi"][e], x["epi"][e], x["epi"][e], x["epi"][e], 0.0, 0.0)
            spec = Spectrum(event=event)
            spec.frequencies = np.array(x["frequencies"])
            spec.phases = ["noise", "p"]
            spec.multi_component_spectrum = True
            present = np.flatnonzero(x["present"][e])
            spec.p_spectrum = {names[s]: {"spectrum": np.array(x["corrected"][e, s]), "freq": spec.frequencies}
                               for s in present}
            spec.snr_p_spectrum = {names[s]: {"snr": np.array(x["snr"][e, s]), "freq": spec.frequencies}
                                   for s in present}
            for o, option in enumerate(sc.MW_OPTIONS):
                seen = {}

                def capture(snr, snr_threshold, **kw):
                    seen["snr"] = snr.copy()
                    seen["weights"] = _snr_based_weights(snr, snr_threshold, **kw).copy()
                    return seen["weights"].copy()

                msnr, raw = np.zeros(S, np.float32), np.zeros(S, np.float32)
                try:
                    with np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
                        value = approximate_moment_magnitude(
                            spec, snr_threshold=sc.THRESHOLD, num_averaging_bands=option[0],
                            low_snr_freq_min_hz=option[1], magnitude_log_moment_scaling=sc.SCALING, phases=["p"],
                            snr_based_weights=capture)["p"]
                    msnr[present], raw[present] = seen["snr"], seen["weights"]
                    raised = False
                except ValueError:
                    value, raised = np.nan, True
                for key, v in (("mw", value), ("msnr", msnr), ("rawweights", raw), ("mwraised", raised)):
                    rows.setdefault(f"{key}_{name}_{o}", [None] * E)[e] = v
        for key, values in rows.items():
            out[key] = np.stack([np.asarray(v) for v in values])
        print(name)
    out["numpy_version"] = np.array(np.__version__)
    out["pandas_version"] = np.array(pd.__version__)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
