"""GPU: every device-pointer entry point run between guard bands, on workspaces of exactly the size its sibling
bpmf_*_workspace_bytes names (tests/arena.py, tests/guard_cases.py).

For every case and every workspace size of the table:
 1. result    status 0 and the outputs equal the entry point's definition under its own comparison;
 2. fence     no byte of any guard changed, in front or behind, with debug.poison_output on (tests/conftest.py);
 3. any workspace   the call on a workspace of 0xFF bytes and on one of 0x00 bytes gives the same bits (a call
    without a workspace runs once: bpmf_bp_extract_peaks_dev stores its records in arbitrary order);
 4. any size  where two sizes are accepted, both give the same bits;
 5. refusal   one byte under the smallest accepted size: status -1, bpmf_last_error names the workspace, and NOTHING
    in the arena changed -- guards, workspace, outputs.  For this run the output bodies hold 0x3C instead of 0xFF, so
    that a poisoning memset issued ahead of the argument checks shows too.

A read past the end of an input meets 0xFF bytes (NaN / -1) and fails the result; a store outside an output or outside
[d_workspace, d_workspace + workspace_bytes) changes a guard."""
import ctypes as C

import numpy as np
import pytest

import arena as ar
import guard_cases as gc

pytestmark = pytest.mark.gpu

REFUSAL_OUTPUT_BYTE = 0x3C


def _lib():
    from seismic_bpmf_amd import _lib
    return _lib.lib()


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def build_arena(call, sizes, fill, output_byte=ar.OUTPUT_BYTE):
    a = ar.Arena("torch")
    for name, value in call.inputs.items():
        a.add_input(name, value)
    for name, spec in call.outputs.items():
        a.add_output(name, spec[0], spec[1], init=spec[2] if len(spec) > 2 else None, fill=output_byte)
    for name, nbytes in sizes.items():                     # last: a slab too many behind it lands in the slack
        a.add_workspace(name, nbytes, fill)
    return a.commit()


def run(call, a, sizes, invoke=None):
    """One call on the arena: (status, message)."""
    import torch
    lib = _lib()
    p = {r.name: C.c_void_p(r.ptr) for r in a.regions}
    rc = (invoke or call.invoke)(lib, p, dict(sizes), _stream())
    torch.cuda.synchronize()
    return rc, lib.bpmf_last_error().decode("utf-8", "replace")


def check_call(call):
    from seismic_bpmf_amd import _lib
    assert _lib.get_option("debug.poison_output")[0] == 1
    bits = {}
    for k, sizes in enumerate(call.variants):
        for fill in (0xFF, 0x00) if sizes else (0xFF,):    # (no workspace: nothing to fill, one run)
            a = build_arena(call, sizes, fill)
            rc, msg = run(call, a, sizes)
            assert rc == 0, (call.name, sizes, msg)
            assert a.check() == [], (call.name, sizes, hex(fill))                          # 2. the fence
            assert not any(r.changed() for r in a.regions if r.kind == "input"), (call.name, "an input was written")
            out = {name: a[name].value() for name in call.outputs}
            call.verify(out)                                                               # 1. the result
            bits[k, fill] = {name: a[name].raw() for name in call.outputs}
            del a
    first = bits[0, 0xFF]
    for key, got in bits.items():                                                         # 3. and 4.
        for name in call.outputs:
            assert np.array_equal(got[name], first[name]), \
                (call.name, name, f"workspace size {key[0]} filled with {key[1]:#x} differs from size 0 filled with 0xff")
    if call.refusal is not None:                                                          # 5. the refusal
        sizes = {**call.variants[-1], **call.refusal}
        a = build_arena(call, sizes, 0xFF, output_byte=REFUSAL_OUTPUT_BYTE)
        rc, msg = run(call, a, sizes, call.refusal_invoke)
        assert rc == -1 and "workspace" in msg and call.entry in msg, (call.name, rc, msg)
        assert a.check() == [] and np.array_equal(a.now(), a.image), (call.name, "refused, yet", a.changed_bodies())


@pytest.mark.parametrize("label,builder", gc.builders(), ids=[b[0] for b in gc.builders()])
def test_between_guard_bands(label, builder, hip_opts):
    lib = _lib()
    calls = builder(lib)
    assert calls
    for call in calls:
        for name, value in call.options.items():
            hip_opts(name, value)
        state = call.before(lib) if call.before else None
        try:
            check_call(call)
        finally:
            if call.after:
                call.after(lib, state)
            for name in call.options:
                hip_opts.reset(name)
