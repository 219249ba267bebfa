"""GPU: the stage subsets of bpmf_source_spectra_dev through the C ABI (include/bpmf_hip.h: `flags` is a bit set).

The Python surface passes flags 7 and 8 only.  Here flags 1, 2, 3, 4, 5, 6, 7, 8, 12 and 15 run on cases `edge` and
`components`, against the 7-then-8 path that the Python surface takes:
 * every output of a stage asked for equals that path's bit for bit;
 * `snr` / `corrected`, where their stage is not asked for but a later one reads them, are filled from a flags-3 call
   beforehand and come back unchanged;
 * every other output buffer keeps its fill of 0x3C bytes, with debug.poison_output on (tests/conftest.py);
 * the pointers that no stage asked for reads or writes are passed as null, and the call succeeds."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import source_spectra_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0x3C
FLAGS = (1, 2, 3, 4, 5, 6, 7, 8, 12, 15)
OPTIONS = dict(average_log=1, median=1, min_num_valid=0, max_err_pct=25.0, bands=2, max_bad=sc.MAX_BAD)


class Buffers:
    """The twelve outputs as device buffers of FILL bytes, and the ten inputs uploaded."""

    def __init__(self, name, phase):
        import torch
        self.torch = torch
        arrays, self.params = sc.c_inputs(name, phase)
        E, S = arrays["valid"].shape
        self.F = len(arrays["frequencies"])
        self.C = arrays["signal"].size // (E * S * self.F)
        self.E, self.S = E, S
        self.params.update(OPTIONS, first_high=int(np.searchsorted(arrays["frequencies"], 2.0, side="right")))
        self.inputs = {k: torch.as_tensor(v, device="cuda") for k, v in arrays.items()}
        self.specs = sc.output_specs(E, S, self.C, self.F)
        self.outputs = {}
        self.refill()

    def refill(self):
        for k, (shape, dtype) in self.specs.items():
            n = int(np.prod(shape)) * np.dtype(dtype).itemsize
            self.outputs[k] = self.torch.full((n,), FILL, dtype=self.torch.uint8, device="cuda")

    def put(self, key, value):
        self.outputs[key] = self.torch.as_tensor(np.ascontiguousarray(value).view(np.uint8).ravel(), device="cuda")

    def call(self, flags, null_untouched=True):
        from seismic_bpmf_amd import _lib
        used, _ = sc.touched(flags)
        tensors = {**self.inputs, **self.outputs}
        p = {k: C.c_void_p(t.data_ptr()) for k, t in tensors.items() if k in used or not null_untouched}
        stream = C.c_void_p(self.torch.cuda.current_stream().cuda_stream)
        rc = sc.c_call(_lib.lib(), p, self.E, self.S, self.C, self.F, flags, stream, **self.params)
        self.torch.cuda.synchronize()
        assert rc == 0, (flags, _lib.lib().bpmf_last_error())

    def get(self):
        out = {}
        for k, (shape, dtype) in self.specs.items():
            out[k] = self.outputs[k].cpu().numpy().view(dtype).reshape(shape)
        return out


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module", params=["edge", "components"])
def case(request):
    """(buffers, the outputs of flags 7 followed by flags 8, as the Python surface calls them)."""
    from seismic_bpmf_amd import _lib
    assert _lib.get_option("debug.poison_output")[0] == 1
    b = Buffers(request.param, "p")
    b.call(7, null_untouched=False)
    b.call(8, null_untouched=False)
    want = b.get()
    for k, v in want.items():                              # every element was written: no fill is left
        assert not (v.view(np.uint8) == FILL).all() or v.size == 0, k
    return b, want


@pytest.mark.parametrize("flags", FLAGS)
def test_a_stage_subset_equals_the_chained_calls(case, flags):
    b, want = case
    b.refill()
    used, written = sc.touched(flags)
    given = [k for k in ("snr", "corrected") if k in used and k not in written]
    for k in given:                                        # an input of stages 4 and 8 when its bit is not set
        b.put(k, want[k])
    b.call(flags)
    got = b.get()
    for k in sc.POINTER_OUTPUTS:
        if k in written or k in given:
            assert same_bits(got[k], want[k]), (flags, k)
        else:
            assert (got[k].view(np.uint8) == FILL).all(), (flags, k, "an output of a stage not asked for was written")


def test_the_flags_3_call_fills_what_stages_4_and_8_read(case):
    b, want = case
    b.refill()
    b.call(3)
    first = b.get()
    assert same_bits(first["snr"], want["snr"]) and same_bits(first["corrected"], want["corrected"])
    b.call(12)                                             # on the buffers the flags-3 call left
    got = b.get()
    for k in sc.POINTER_OUTPUTS:
        assert same_bits(got[k], want[k]), k
