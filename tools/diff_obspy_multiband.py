#!/usr/bin/env python3
"""First-contact kit for the multi-band spectra: diff REAL obspy against the definition's restatement of it.

Spectrum.compute_multi_band_spectrum (BPMF/spectrum.py:387-505) runs three obspy operations on every trace and band:
tr.detrend("constant") / tr.detrend("linear"), tr.taper(0.25, max_length=buffer_seconds, type="cosine") and
tr.filter("bandpass", corners=, zerophase=True).  obspy was not installed where postprocess.multiband_spectrum_host was
written; the three were restated from obspy's documented behaviour (scipy.signal.detrend; a half-Hann of
w = min(int(0.25 npts), int(max_length sr)) samples on each side; iirfilter -> zpk2sos -> sosfilt forward and on the
reversed output), and tests/golden/multiband.npz pins only the reference's logic AROUND them (duck-typed traces).  THIS
script settles the three themselves on a machine that has obspy:

    python tools/diff_obspy_multiband.py                      # needs obspy; prints the deviation per operation
    BPMF_RECORD_REFERENCE=<tree> python tools/diff_obspy_multiband.py    # also the reference on real obspy.Trace objects

Per case of tests/multiband_cases.py (the rows that are neither zero, constant nor hold a NaN) it prints the worst
deviation, relative to the largest sample that goes into the filter, of
    detrend   obspy's two detrends of a float64 trace     against steps 1-2 of the definition,
    taper     obspy's taper of a trace of ones            against the definition's window (absolute),
    filter    obspy's zero-phase band-pass of the definition's prepared row, per band
                                                          against the definition's cascade,
    whole     (with the reference tree) compute_multi_band_spectrum on obspy.Trace objects
                                                          against multiband_spectrum_host, in the measure of
                                                          multiband_cases.deviation,
and exits 1 if one of them exceeds --limit (default: the `limit` of tests/golden/multiband.npz; the taper: 1e-15).
tests/test_multiband_obspy_live.py asserts the same under pytest.importorskip("obspy")."""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

TAPER_LIMIT = 1e-15


def trace(data, sr, station="ST00", channel="HH0"):
    from obspy import Trace
    return Trace(data=np.array(data), header={"sampling_rate": sr, "network": "XX", "station": station,
                                               "channel": channel})


def operation_deviations(index):
    """{"detrend", "taper", "filter"}: the worst deviations of real obspy from the definition on CASES[index]."""
    import multiband_cases as mc
    from seismic_bpmf_amd import postprocess as pp
    _, n, buffer_seconds, corners, band_key, _ = mc.CASES[index]
    sr, bands = mc.SAMPLING_RATE, mc.BANDS[band_key]
    x = mc.windows(index)[mc.live_rows(mc.windows(index))][:6]          # a few live rows
    plan = pp.multiband_plan(n, bands, sr, buffer_seconds, corners)
    w, out = plan["taper"], {"detrend": 0.0, "taper": 0.0, "filter": 0.0}
    ones = trace(np.ones(n), sr)
    ones.taper(0.25, max_length=buffer_seconds, type="cosine")
    mine = np.ones(n)
    if w:
        g = 0.5 * (1.0 - np.cos(np.pi * np.arange(w, dtype=np.float64) / w))
        mine[:w], mine[n - w:] = g, g[::-1]
    out["taper"] = float(np.abs(np.asarray(ones.data, dtype=np.float64) - mine).max())
    bare, prepared = pp.multiband_prepare_host(x, 0), pp.multiband_prepare_host(x, w)
    for r in range(len(x)):
        tr = trace(x[r].astype(np.float64), sr)
        tr.detrend("constant")
        tr.detrend("linear")
        top = np.abs(bare[r]).max()
        out["detrend"] = max(out["detrend"], float(np.abs(tr.data - bare[r]).max() / top))
        top = np.abs(prepared[r]).max()
        for b, (lo, hi) in enumerate(plan["bands"]):
            if plan["skip"][b]:
                continue
            tr = trace(prepared[r], sr)
            tr.filter("bandpass", freqmin=lo, freqmax=hi, corners=corners, zerophase=True)
            y = pp.sosfilt_rows(plan["sos"][b], prepared[r][None])
            y = pp.sosfilt_rows(plan["sos"][b], y[:, ::-1])[0, ::-1]
            out["filter"] = max(out["filter"], float(np.abs(tr.data - y).max() / top))
    return out


def reference_spectrum():
    """BPMF.spectrum.Spectrum from the tree BPMF_RECORD_REFERENCE names, or None."""
    ref = os.environ.get("BPMF_RECORD_REFERENCE")
    if not ref:
        return None
    spec = importlib.util.spec_from_file_location("make_goldens", os.path.join(ROOT, "tests", "golden",
                                                                               "make_goldens.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    mg.REF = ref
    cwd = os.getcwd()
    try:
        mg.import_reference()
    finally:
        os.chdir(cwd)
    from BPMF.spectrum import Spectrum
    return Spectrum


def whole_deviation(Spectrum, index):
    """The reference on real obspy.Trace objects (float64 data) against the definition, on CASES[index]; the row that
    holds a NaN is left out (scipy.signal.detrend refuses it)."""
    import multiband_cases as mc
    from seismic_bpmf_amd import postprocess as pp
    _, n, buffer_seconds, corners, band_key, (E, S, C) = mc.CASES[index]
    sr, bands = mc.SAMPLING_RATE, mc.BANDS[band_key]
    x = mc.windows(index)
    mine, _ = pp.multiband_spectrum_host(x, bands, sr=sr, buffer_seconds=buffer_seconds, corners=corners)
    plan = pp.multiband_plan(n, bands, sr, buffer_seconds, corners)
    prepared = pp.multiband_prepare_host(x.reshape(-1, n), plan["taper"]).reshape(x.shape)
    ref = np.zeros_like(mine)

    class Distances:
        loc = type("Loc", (), {"__getitem__": lambda self, key: 10.0})()

    class Event:
        hmax_unc, vmax_unc, source_receiver_dist = 1.0, 1.0, Distances()

    for e in range(E):
        traces = [trace(x[e, s, c].astype(np.float64), sr, f"ST{s:02d}", f"HH{c}") for s in range(S) for c in range(C)
                  if not np.isnan(x[e, s, c]).any()]
        spec = Spectrum(event=Event())
        spec.set_frequency_bands(dict(bands))
        spec.compute_multi_band_spectrum(traces, "p", buffer_seconds, corners=corners)
        for s in range(S):
            for c in range(C):
                key = f"XX.ST{s:02d}..HH{c}"
                ref[e, s, c] = spec.p_spectrum[key]["spectrum"] if key in spec.p_spectrum else mine[e, s, c]
    return mc.deviation(mine, ref, mc.row_scale(x, prepared), bands)


def main():
    import golden_npz
    import multiband_cases as mc
    ap = argparse.ArgumentParser()
    ap.add_argument("--limit", type=float, default=None)
    ap.add_argument("--cases", type=int, nargs="+", default=list(range(len(mc.CASES) - 1)))
    args = ap.parse_args()
    try:
        import obspy
    except ImportError as exc:
        print(f"obspy does not import here ({exc}); nothing to diff")
        return 2
    limit = args.limit
    if limit is None:
        limit = float(golden_npz.load(os.path.join(ROOT, "tests", "golden", "multiband.npz"))["limit"])
    Spectrum = reference_spectrum()
    print(f"obspy {obspy.__version__}; limit {limit:.3e}; reference tree: {'yes' if Spectrum else 'no (whole: skipped)'}")
    bad = False
    for index in args.cases:
        dev = operation_deviations(index)
        if Spectrum is not None:
            dev["whole"] = whole_deviation(Spectrum, index)
        print(f"{mc.CASES[index][0]}: " + ", ".join(f"{k} {v:.2e}" for k, v in dev.items()))
        bad = bad or dev["taper"] > TAPER_LIMIT or any(v > limit for k, v in dev.items() if k != "taper")
    print("DIFFERENT: the restatement of obspy's operations does not hold" if bad else
          "the three obspy operations equal their restatement within the limit")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
