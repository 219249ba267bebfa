"""CPU, only where obspy is installed: the three obspy operations the reference's multi-band spectra rest on --
Trace.detrend("constant" / "linear"), Trace.taper(0.25, max_length=, type="cosine") and Trace.filter("bandpass",
corners=, zerophase=True) -- against their restatement in postprocess.multiband_spectrum_host
(tools/diff_obspy_multiband.py has the comparison; this file asserts it).  With BPMF_RECORD_REFERENCE naming the
reference tree, Spectrum.compute_multi_band_spectrum itself runs on real obspy.Trace objects.

SKIPPED where obspy does not import: the definition was written without obspy at hand, from its documentation, and
tests/golden/multiband.npz pins only the reference's logic around the three operations (duck-typed traces).  Until this
file has run next to a real obspy the three operations themselves are unverified."""
import importlib.util
import os
import sys

import pytest

pytest.importorskip("obspy", reason="obspy is not installed: the restatement of its detrend / taper / filter in "
                                    "postprocess.multiband_spectrum_host stays unverified here "
                                    "(tools/diff_obspy_multiband.py)")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import golden_npz  # noqa: E402
import multiband_cases as mc  # noqa: E402

_spec = importlib.util.spec_from_file_location("diff_obspy_multiband", os.path.join(ROOT, "tools",
                                                                                    "diff_obspy_multiband.py"))
kit = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kit)

LIMIT = float(golden_npz.load(os.path.join(ROOT, "tests", "golden", "multiband.npz"))["limit"])
CASES = [1, 2, 3, 4, 5, 8, 9, 11]


@pytest.mark.parametrize("index", CASES, ids=[mc.CASES[i][0] for i in CASES])
def test_obspy_operations_equal_their_restatement(index):
    dev = kit.operation_deviations(index)
    print(mc.CASES[index][0], dev)
    assert dev["taper"] <= kit.TAPER_LIMIT, dev
    assert dev["detrend"] <= LIMIT and dev["filter"] <= LIMIT, dev


@pytest.mark.parametrize("index", CASES, ids=[mc.CASES[i][0] for i in CASES])
def test_reference_on_obspy_traces_equals_the_definition(index):
    Spectrum = kit.reference_spectrum()
    if Spectrum is None:
        pytest.skip("BPMF_RECORD_REFERENCE does not name the reference tree")
    dev = kit.whole_deviation(Spectrum, index)
    assert dev <= LIMIT, dev
