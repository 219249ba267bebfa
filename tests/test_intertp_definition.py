"""CPU: the float64 definition of the inter-template CC (tests/f64_anchor.py: intertp_f64, B_sym) judged on its own, and
the SENSITIVITY of the GPU checks that rest on it (tests/test_gpu_intertp_anchor.py).

  * on every shape and regime the GPU tests run, the composition of the C oracle (the matched filter per data template
    with network_sum=False, then np.max over the lags, np.sum over the channels and the symmetrisation -- what
    test_intertemplate_cc_against_oracle builds) lies within B_raw / B_sym of the definition, and is exactly +0 wherever
    the definition computes nothing;
  * every case holds what intertp_case promises for its T;
  * the definition with a planted defect (intertp_f64's `drop`) leaves its own bound on the cases the table below names --
    a condition on the cases, not a measurement: a defect that no case catches means the cases are too weak.
"""
import functools

import numpy as np
import pytest

import f64_anchor as fa

OVERFLOW = ("LDS overflow", (2, 1, 1, 17000, 0))          # one channel beyond the batched launch's LDS budget: the loop
CASES = [(row, regime) for row in fa.INTERTP_ROWS for regime in fa.intertp_regimes_of(row)]


@functools.lru_cache(maxsize=None)
def _evaluated(row, regime):
    shape = fa.INTERTP_ROWS.get(row, OVERFLOW[1])
    args = fa.intertp_case(regime, *shape, seed=fa.intertp_seed(row) if row in fa.INTERTP_ROWS else 4999)
    return args, fa.intertp_f64(*args, shape[4], exact=regime == "int")


def oracle_composition(oracle_lib, wf, base, mask, max_lag):
    """(raw, sym) float32, built as the reference builds them (dataset.py:4818-4833) around the oracle's matched filter."""
    T, S, C, Lw = wf.shape
    raw = np.zeros((T, T), dtype=np.float32)
    trimmed = np.ascontiguousarray(wf[..., max_lag:Lw - max_lag])
    for t in range(T):
        w = (base[t][None] * mask[t][:, None, None]).astype(np.float32)
        keep = np.flatnonzero((w != 0).reshape(T, -1).sum(axis=1) > 0)
        if keep.size == 0:
            continue
        cc = oracle_lib.matched_filter(trimmed[keep], np.zeros((keep.size, S, C), np.int32), w[keep], wf[t], 1,
                                       network_sum=False)
        raw[t, keep] = np.sum(w[keep] * np.max(cc, axis=1), axis=(-1, -2))
    return raw, (raw + raw.T) / 2.0


# ------------------------------------------------------------------------------ the pieces ---
def test_lds_chunks_follow_the_budget_and_the_host_route_follows_the_same_rule():
    from seismic_bpmf_amd import workflow
    for row, chunks in fa.INTERTP_CHUNKS.items():
        T, S, C, Lw, m = fa.INTERTP_ROWS[row]
        c = fa.intertp_lds_chunk(S * C, Lw, m)
        assert (c, S * C - c) == chunks and S * C <= 2 * c, row
    assert fa.intertp_lds_chunk(136, 96, 5) == 83 and fa.intertp_lds_chunk(9, 96, 16) == 9
    assert fa.intertp_lds_chunk(1, 17000, 0) == 0 and fa.intertp_lds_chunk(1, 16368, 0) == 1 and fa.intertp_lds_chunk(1, 16369, 0) == 0
    for n_ch in (1, 3, 137, 1500, 2047, 2048):
        for Lw in (1, 96, 2078, 15000, 16000, 16368, 16369, 17000):
            for m in (0, 5, 31, 32):
                if Lw > 2 * m:
                    assert workflow.intertp_batched_fits(n_ch, Lw, m) == (m <= fa.INTERTP_MAX_LAG and fa.intertp_lds_chunk(n_ch, Lw, m) >= 1)


@pytest.mark.parametrize("row,regime", CASES)
def test_cases_hold_what_they_promise(row, regime):
    T, S, C, Lw, m = fa.INTERTP_ROWS[row]
    args, ref = _evaluated(row, regime)
    L, n_ch = Lw - 2 * m, S * C
    f = fa.intertp_features(args, ref, m)
    print(f"{row} {regime}: {f}")
    wide = L >= 7                                                 # (a window of a few samples correlates with anything)
    assert f["last_lag_best"] == (T > 1) or not wide
    assert f["first_lag_best"] == (T > 2) or not wide
    assert f["negated"] == (T > 3) or not wide or regime == "sine"      # (a sinusoid meets its negative half a period on)
    assert f["dead_channel"] == (n_ch >= 2 or T > 5)
    assert f["unweighted_row"] == (T > 4) and f["empty_mask_row"] == (T > 6)
    assert f["asymmetric_mask"] >= min(3, max(0, T - 2)) and f["rows_differ"] == (T > 1)
    # the exact zeros the issue names are inside ref.zero, and the matrix is not all zeros
    wf, w, mask = args
    assert ref.zero[~mask].all() and ref.zero[~(w.reshape(T, -1) != 0).any(axis=1)].all() and not ref.zero.all()


# ------------------------------------------------------------------------------ the definition ---
@pytest.mark.parametrize("row", list(fa.INTERTP_ROWS) + [OVERFLOW[0]])
def test_oracle_composition_lies_within_the_bound(oracle_lib, row):
    shape = fa.INTERTP_ROWS.get(row, OVERFLOW[1])
    for regime in fa.intertp_regimes_of(row):
        args, ref = _evaluated(row, regime)
        raw, sym = oracle_composition(oracle_lib, *args, shape[4])
        fa.intertp_compare(sym, ref, raw=raw, what=f"oracle composition {row} {shape} {regime}").require()


def test_the_checker_rejects_an_entry_beyond_its_bound_and_a_zero_that_is_not_plus_zero(oracle_lib):
    row = "4 33 lags, 9 channels, three tiles"
    args, ref = _evaluated(row, "noise")
    raw, sym = oracle_composition(oracle_lib, *args, fa.INTERTP_ROWS[row][4])
    assert fa.intertp_compare(sym, ref, raw=raw).n_bad == 0
    t, u = (int(x) for x in np.argwhere(ref.B_sym > 0)[-1])
    off = sym.copy()
    off[t, u] += np.float32(3 * ref.B_sym[t, u])
    assert fa.intertp_compare(off, ref, raw=raw).n_bad == 1
    t, u = (int(x) for x in np.argwhere(ref.zero)[0])
    for junk in (np.float32(-0.0), np.float32(1e-30), np.float32(np.nan)):
        bad = raw.copy()
        bad[t, u] = junk
        assert fa.intertp_compare(sym, ref, raw=bad).n_bad == 1, junk


# ------------------------------------------------------------------------------ sensitivity ---
def _expected(drop, T, S, C, Lw, m):
    """Whether a case of this shape must catch the defect (None: either way).  The lag and trim defects need a pair whose
    best lag is the last / the first one (templates 1 and 2) and a window wide enough for that maximum to stand alone;
    "tail" and "lds_chunk" change something exactly where L % 8 != 0 / the channels span several LDS passes; "w_u" and
    "no_sym" need two templates, "mask_T" the pair (1, 2), "abs_max" the negated template."""
    L, n_ch = Lw - 2 * m, S * C
    wide = L >= 7
    if drop == "first_lag":
        return True if (T > 2 and m >= 1 and wide) else (False if m == 0 else None)
    if drop in ("last_lag", "trim"):
        return True if (T > 1 and m >= 1 and wide) else (False if m == 0 else None)
    if drop == "tail":
        return L % 8 != 0
    if drop == "abs_max":
        return True if T > 3 else None
    if drop in ("w_u", "no_sym"):
        return T > 1
    if drop == "mask_T":
        return True if T > 2 else False
    if drop == "last_channel":
        return True
    assert drop == "lds_chunk"
    return fa.intertp_lds_chunk(n_ch, Lw, m) < n_ch


def _outside(variant, ref):
    """Entries of the defective definition that the checks of the GPU tests reject: beyond B_sym, beyond B_raw, or not
    zero where raw must be."""
    return int((~(np.abs(variant.sym - ref.sym) <= ref.B_sym)).sum() + (~(np.abs(variant.raw - ref.raw) <= ref.B_raw)).sum())


@pytest.mark.parametrize("regime", ["noise", "int"])
def test_a_planted_defect_fails_the_checks_of_the_gpu_tests(regime):
    caught = {drop: [] for drop in fa.INTERTP_DROPS}
    for row, shape in fa.INTERTP_ROWS.items():
        args, ref = _evaluated(row, regime)
        marks = []
        for drop in fa.INTERTP_DROPS:
            n = _outside(fa.intertp_f64(*args, shape[4], exact=regime == "int", drop=drop), ref)
            want = _expected(drop, *shape)
            assert want is None or (n > 0) == want, (row, regime, drop, n)
            marks.append(f"{drop}:{n}")
            if n:
                caught[drop].append(row.split()[0])
        print(f"sensitivity {regime} {row}: entries outside -- " + " ".join(marks))
    for drop, rows in caught.items():
        print(f"sensitivity {regime}: {drop} caught by rows {' '.join(sorted(set(rows), key=lambda r: (len(r), r)))}")
        assert rows, drop
