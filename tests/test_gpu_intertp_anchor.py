"""GPU: the batched inter-template CC (csrc/intertp.hip through workflow.intertemplate_cc) and the per-template loop
(workflow.intertemplate_cc_loop) against the float64 definition of tests/f64_anchor.py -- the oracle is not in the loop.

Every row of fa.INTERTP_ROWS enters a corner of the kernel's parameter range: 63 lags in 8 lag groups, template lengths
around the 8-sample block loop and its tail, channel counts on both sides of every branch of the NumPy-order sum (7 / 8 /
9, 128 / 129 / 136 / 137), channels split over several LDS passes (and exactly two full ones), waveforms across the
1024-sample chunks of the window energies' prefix sums, one sample, one template.  Per case: the batched result and the
loop's within B_sym (before the symmetrisation: within B_raw, exact +0 where the definition computes nothing), and the two
bit-equal.  Then what no bound sees: permuting or appending templates must not change a bit of the other entries; the C
entry point refuses what it cannot take without touching the output; a channel beyond the LDS budget takes the loop.
Every check prints its worst err / B (pytest -rP shows them).
"""
import ctypes as C

import numpy as np
import pytest

import f64_anchor as fa

pytestmark = pytest.mark.gpu

TABLE = [r for r in fa.INTERTP_ROWS if not r.startswith("12 ")]
ROW4, ROW5 = "4 33 lags, 9 channels, three tiles", "5 129 channels"


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _judge(row, regime, shape=None, batched=True):
    from seismic_bpmf_amd import workflow
    T, S, Cc, Lw, m = shape or fa.INTERTP_ROWS[row]
    args = fa.intertp_case(regime, T, S, Cc, Lw, m, seed=fa.intertp_seed(row) if row in fa.INTERTP_ROWS else 4999)
    wf, base, mask = args
    ref = fa.intertp_f64(*args, m, exact=regime == "int")
    assert workflow.intertp_batched_fits(S * Cc, Lw, m) == batched
    what = f"{row} {(T, S, Cc, Lw, m)} {regime}"
    raw = workflow.intertemplate_cc(wf, base, max_lag=m, pair_mask=mask, symmetrise=False)
    sym = workflow.intertemplate_cc(wf, base, max_lag=m, pair_mask=mask)
    fa.intertp_compare(sym, ref, raw=raw, what=f"kernel intertp {what}").require()
    full = base[:, None, :, :] * mask[:, :, None, None]
    raw_loop = workflow.intertemplate_cc_loop(wf, full, max_lag=m, symmetrise=False)
    sym_loop = workflow.intertemplate_cc_loop(wf, full, max_lag=m)
    fa.intertp_compare(sym_loop, ref, raw=raw_loop, what=f"loop intertp {what}").require()
    assert np.array_equal(_bits(raw), _bits(raw_loop)) and np.array_equal(_bits(sym), _bits(sym_loop)), what
    assert np.array_equal(_bits(sym), _bits((raw + raw.T) / 2.0)), what


def test_the_lds_passes_of_the_table_follow_the_launchers_budget():
    """The premise of rows 5, 7 and 8: the launcher stages as many channels per pass as fit 64 KB beside the CCs of a tile
    of 8 templates and their weighted maxima -- ch_chunk * Lw + 8 * ch_chunk * n_lag + 8 * n_ch floats
    (fa.intertp_lds_chunk).  A change of that budget fails here, not in the kernel checks."""
    for row, chunks in fa.INTERTP_CHUNKS.items():
        T, S, Cc, Lw, m = fa.INTERTP_ROWS[row]
        c = fa.intertp_lds_chunk(S * Cc, Lw, m)
        assert (c, S * Cc - c) == chunks, (row, c)
        assert 4 * (c * Lw + 8 * c * (2 * m + 1) + 8 * S * Cc) <= 64 * 1024 < 4 * ((c + 1) * Lw + 8 * (c + 1) * (2 * m + 1) + 8 * S * Cc)


@pytest.mark.parametrize("row", TABLE, ids=lambda r: r.split()[0])
def test_table_rows_against_the_definition(row):
    for regime in fa.intertp_regimes_of(row):
        _judge(row, regime)


@pytest.mark.parametrize("m", [3, 4, 7, 8, 28])
def test_lag_groups_and_block_remainders_against_the_definition(m):
    """Row 12: 7, 9, 15, 17 and 57 lags against the groups of 8 lags, L = 7, 9, 15, 16 against the blocks of 8 samples."""
    for L in (7, 9, 15, 16):
        for regime in ("noise", "int"):
            _judge(f"12 m={m} L={L}", regime)


def test_a_channel_beyond_the_lds_budget_takes_the_loop():
    for regime in ("noise", "int"):
        _judge("LDS overflow", regime, shape=(2, 1, 1, 17000, 0), batched=False)


# ------------------------------------------------------------------------------ bitwise properties ---
def _both(wf, base, mask, m):
    from seismic_bpmf_amd import workflow
    return (workflow.intertemplate_cc(wf, base, max_lag=m, pair_mask=mask, symmetrise=False),
            workflow.intertemplate_cc(wf, base, max_lag=m, pair_mask=mask))


@pytest.mark.parametrize("row", [ROW4, ROW5], ids=lambda r: r.split()[0])
def test_permuting_the_templates_permutes_the_matrix_bit_for_bit(row):
    T, S, Cc, Lw, m = fa.INTERTP_ROWS[row]
    wf, base, mask = fa.intertp_case("noise", T, S, Cc, Lw, m, seed=fa.intertp_seed(row))
    raw, sym = _both(wf, base, mask, m)
    perm = np.concatenate([np.arange(1, T, 2), np.arange(0, T, 2)])      # across the tiles of 8 and into other slots of them
    assert sorted(perm) == list(range(T)) and (perm // 8 != np.arange(T) // 8).sum() >= T // 2 and (perm % 8 != np.arange(T) % 8).sum() >= T // 2
    raw_p, sym_p = _both(wf[perm], base[perm], mask[np.ix_(perm, perm)], m)
    assert np.array_equal(_bits(raw_p), _bits(raw[np.ix_(perm, perm)])), row
    assert np.array_equal(_bits(sym_p), _bits(sym[np.ix_(perm, perm)])), row


@pytest.mark.parametrize("row", [ROW4, ROW5], ids=lambda r: r.split()[0])
def test_appending_templates_leaves_the_block_bit_identical(row):
    T, S, Cc, Lw, m = fa.INTERTP_ROWS[row]
    wf, base, mask = fa.intertp_case("noise", T, S, Cc, Lw, m, seed=fa.intertp_seed(row))
    raw, sym = _both(wf, base, mask, m)
    rng = np.random.default_rng(77)
    for extra in (1, 7, 8):
        wf2 = np.concatenate([wf, rng.standard_normal((extra, S, Cc, Lw)).astype(np.float32)])
        base2 = np.concatenate([base, rng.uniform(0.1, 1.0, (extra, S, Cc)).astype(np.float32)])
        mask2 = rng.random((T + extra, T + extra)) < 0.7
        mask2[:T, :T] = mask
        raw2, sym2 = _both(wf2, base2, mask2, m)
        assert np.array_equal(_bits(raw2[:T, :T]), _bits(raw)) and np.array_equal(_bits(sym2[:T, :T]), _bits(sym)), (row, extra)
        assert np.abs(raw2[T:, :]).max() > 0.01 and np.abs(raw2[:, T:]).max() > 0.01


# ------------------------------------------------------------------------------ the C entry point ---
def test_c_entry_point_refuses_bad_arguments_and_leaves_the_output_untouched():
    import torch
    from seismic_bpmf_amd import _lib, workflow
    lib = _lib.lib()
    T, S, Cc, Lw = 5, 2, 3, 70                             # (Lw > 2 * 32: of max_lag = 32 only the lag count is refused)
    wf_h, base_h, mask_h = fa.intertp_case("noise", T, S, Cc, Lw, 5, seed=3)
    dev = torch.device("cuda")
    wf, base = torch.as_tensor(wf_h, device=dev), torch.as_tensor(base_h, device=dev)
    mask = torch.as_tensor(mask_h.astype(np.uint8), device=dev)
    long_wf = torch.zeros((2, 1, 1, 17000), device=dev)
    FILL = 7.5

    def call(T_=T, Lw_=Lw, m_=5, short=0, null=None, wf_=wf):
        ws = torch.empty(max(1, lib.bpmf_intertemplate_workspace_bytes(max(T_, 1), S, Cc, m_)), dtype=torch.uint8, device=dev)
        out = torch.full((T, T), FILL, device=dev)
        ptr = {"wf": wf_.data_ptr(), "base": base.data_ptr(), "mask": mask.data_ptr(), "ws": ws.data_ptr(), "out": out.data_ptr()}
        if null:
            ptr[null] = None
        n = (1, 1) if wf_ is long_wf else (S, Cc)
        rc = lib.bpmf_intertemplate_cc_dev(ptr["wf"], ptr["base"], ptr["mask"], T_, n[0], n[1], Lw_, m_, ptr["ws"],
                                           ws.numel() - short, C.c_void_p(torch.cuda.current_stream().cuda_stream), ptr["out"])
        torch.cuda.synchronize()
        return rc, out.cpu().numpy()

    refused = {f"null {k}": dict(null=k) for k in ("wf", "base", "mask", "ws", "out")}
    refused.update({"T = 0": dict(T_=0), "max_lag = 32": dict(m_=32), "Lw = 2 max_lag": dict(Lw_=10),
                    "workspace one byte short": dict(short=1),
                    "a channel beyond the LDS budget": dict(T_=2, Lw_=17000, m_=0, wf_=long_wf)})
    for name, kw in refused.items():
        rc, out = call(**kw)
        err = _lib.last_error()
        print(f"{name}: {rc}, {err!r}")
        assert rc == -1 and "bpmf_intertemplate_cc_dev" in err, (name, rc, err)
        assert (out == FILL).all(), name
    rc, out = call()
    assert rc == 0
    want = workflow.intertemplate_cc(wf_h, base_h, max_lag=5, pair_mask=mask_h, symmetrise=False)
    assert np.array_equal(_bits(out), _bits(want))
