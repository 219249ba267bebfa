"""Which kernel a matched-filter call of the GPU tests takes (bpmf_mf_launch_info).  Every kernel family gives the
same bits, so a test that sets an option in order to reach a family proves nothing about that family unless it
also asserts that the family is what its shape takes."""
from seismic_bpmf_amd import _lib


def assert_takes(templates_shape, N, step=1, network_sum=True, flags=0, **fields):
    """Launches of these templates take a kernel with these fields of _lib.mf_launch_info under the current
    options -- of 1 .. T of them: the host-pointer call cuts the templates into batches, and several devices
    share them."""
    T, S, C, L = templates_shape
    for t in range(1, T + 1):
        info = _lib.mf_launch_info(step, L, N, t, S, C, network_sum, flags)
        assert info["refusal"] is None, info
        for name, value in fields.items():
            assert info[name] == value, (name, value, t, info)
