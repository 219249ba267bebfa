"""CPU: the host side of the batched event relocation (workflow.relocate_events) -- the focus rule that turns a
per-sample maximum over the sources into the first maximum of the volume (postprocess.focus_from_max, the
mirror of the focus kernel of csrc/bp_relocate.hip), and the argument checks that need no device."""
import types

import numpy as np
import pytest

from seismic_bpmf_amd import postprocess as pp, workflow


def running_max(vol):
    """(maxbeam, arg) of a (K, N) volume by the build's convention (oracle/bpmf_oracle.c:bp_cpu): start at
    (0, source 0), sources ascending, replaced on strictly greater."""
    K, N = vol.shape
    best = np.zeros(N, vol.dtype)
    arg = np.zeros(N, np.int32)
    for k in range(K):
        better = vol[k] > best
        best[better] = vol[k][better]
        arg[better] = k
    return best, arg


def seeded_volume(seed):
    """Small non-negative integer-valued volumes: few distinct values, so the maximum is often tied -- across
    sources, across times or both -- and some source rows in front of the winner are all zero."""
    rng = np.random.default_rng(seed)
    K, N = int(rng.integers(2, 9)), int(rng.integers(2, 13))
    if seed % 97 == 0:
        return np.zeros((K, N), np.float32)
    vol = rng.integers(0, int(rng.integers(2, 5)), size=(K, N)).astype(np.float32)
    vol[rng.random(K) < 0.3] = 0.0                       # all-zero source rows
    return vol


def test_focus_from_max_is_the_first_maximum_of_the_volume():
    tied_sources = tied_times = zero_row_first = all_zero = 0
    for seed in range(3000):
        vol = seeded_volume(seed)
        k, t = np.unravel_index(vol.argmax(), vol.shape)
        m = vol.max()
        at = vol == m
        all_zero += int(m == 0)
        if m > 0:
            tied_sources += int(at.any(axis=1).sum() > 1)
            tied_times += int(at.any(axis=0).sum() > 1)
            zero_row_first += int(any(not vol[j].any() for j in range(k)))
        maxbeam, arg = running_max(vol)
        src_idx, time_idx, top = pp.focus_from_max(maxbeam, arg)
        assert (src_idx, time_idx) == (int(k), int(t)) and top == m, (seed, vol)
    # the cases the rule is there for are in the seeds (a condition of this test)
    assert tied_sources >= 50 and tied_times >= 50 and zero_row_first >= 50 and all_zero >= 1


def test_focus_from_max_takes_the_lowest_source_before_the_earliest_time():
    # source 1 reaches the maximum at t = 0, source 0 only at t = 3: source-major order finds source 0 first
    vol = np.array([[0, 1, 0, 5], [5, 0, 0, 0]], np.float32)
    assert np.unravel_index(vol.argmax(), vol.shape) == (0, 3)
    assert pp.focus_from_max(*running_max(vol))[:2] == (0, 3)
    # equal beams at one sample: the arg-max holds the lower source
    vol = np.array([[0, 0, 2], [0, 7, 2], [0, 7, 0]], np.float32)
    assert pp.focus_from_max(*running_max(vol))[:2] == (1, 1)


def fake_beamformer(S=4, P=2, K=10):
    """relocate_events checks its arguments before it touches the beamformer's device."""
    return types.SimpleNamespace(S=S, P=P, K=K)


def test_relocate_events_refuses_windows_outside_the_day():
    day = np.zeros((4, 3, 1000), np.float32)
    wp = np.ones((4, 3, 2), np.float32)
    for starts in ([0, 901], [-1, 10], [1000]):
        with pytest.raises(ValueError, match="leaves the day"):
            workflow.relocate_events(fake_beamformer(), day, wp, starts=starts, n_samples=100)


def test_relocate_events_checks_the_two_input_forms():
    bf = fake_beamformer()
    wp = np.ones((4, 3, 2), np.float32)
    day = np.zeros((4, 3, 1000), np.float32)
    batch = np.zeros((5, 4, 3, 200), np.float32)
    with pytest.raises(ValueError, match="n_samples"):
        workflow.relocate_events(bf, day, wp, starts=[0, 10])                     # starts without n_samples
    with pytest.raises(ValueError, match="n_samples"):
        workflow.relocate_events(bf, batch, wp, n_samples=200)                    # n_samples without starts
    with pytest.raises(ValueError, match=r"\(E, S, C, N\)"):
        workflow.relocate_events(bf, day, wp)                                     # a day is not a batch
    with pytest.raises(ValueError, match="the day"):
        workflow.relocate_events(bf, batch, wp, starts=[0], n_samples=100)        # a batch is not a day
    with pytest.raises(ValueError, match="integer"):
        workflow.relocate_events(bf, day, wp, starts=[0.5], n_samples=100)
    with pytest.raises(ValueError, match="vector"):
        workflow.relocate_events(bf, day, wp, starts=[[0, 1]], n_samples=100)
    with pytest.raises(ValueError, match="at least 1"):
        workflow.relocate_events(bf, day, wp, starts=[0], n_samples=0)
    with pytest.raises(ValueError, match="uncertainty_method"):
        workflow.relocate_events(bf, batch, wp, uncertainty_method="both")
    with pytest.raises(ValueError, match="out_of_bounds"):
        workflow.relocate_events(bf, batch, wp, out_of_bounds="wrap")
    with pytest.raises(ValueError, match="stations"):
        workflow.relocate_events(fake_beamformer(S=5), batch, wp)
    with pytest.raises(ValueError, match="weights_phases"):
        workflow.relocate_events(bf, batch, np.ones((4, 3, 3), np.float32))
