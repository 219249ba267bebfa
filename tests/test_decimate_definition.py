"""CPU: the NumPy definition of the grid decimation (decimate_cases.definition; BPMF/libc.c:55-387) against the oracle,
against the reference's own recorded answers (tests/golden/similar_sources_edges.npz, written by
tests/golden/make_similar_sources_edges_golden.py, and the older similar_sources.npz), and the sharpness of the case
list that tests/test_gpu_decimate.py runs on the device: every planted defect changes the answer of every case that
names it.  `pytest tests/test_decimate_definition.py -rP` prints the matrix defect x cases that reject it."""
import os

import numpy as np
import pytest

import decimate_cases as dc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def answers():
    """The definition's answer to every case and method, computed once and never modified."""
    out = {}
    for case in dc.named_cases() + dc.random_cases():
        for method in dc.METHODS:
            red = dc.definition(*dc.args_of(case), method)
            red.setflags(write=False)
            out[case["name"], method] = red
    return out


@pytest.fixture(scope="module")
def recorded():
    with np.load(os.path.join(GOLD, "similar_sources_edges.npz")) as g:
        return {k: g[k] for k in g.files}


def _recorded_flags(recorded, case, method):
    return np.unpackbits(recorded[f"{case['name']}/{method}"])[:len(case["lon"])].astype(bool)


def test_case_list_is_the_documented_one():
    names = [c["name"] for c in dc.named_cases()]
    for group in (("rounding_closest_f32_square", "rounding_closest_f64_acc", "rounding_smallest_f64_acc",
                   "thr2_rounding", "smallest_add_order", "tie_at_threshold", "tied_ranking", "ranking_asymmetric"),
                  ("chain_in_batch", "chain_across_batches", "chain_shuffled", "chain_in_one_cell"),
                  ("batch_exact_256", "batch_257", "batch_exact_in_cell", "thr0", "thr_big"),
                  ("cells_change_answer", "on_vertices", "outside_cells", "nan_coordinates", "descending_vertices",
                   "one_cell", "many_empty_cells"),
                  ("S1", "K1", "K2_redundant", "K2_kept", "S256_all", "S256_some", "S80", "n_diff_1"),
                  ("nan_moveouts", "negative_threshold", "nan_threshold", "large_offsets", "denormal_differences")):
        assert not set(group) - set(names), set(group) - set(names)
    assert set(dc.DEGENERATE) <= set(names) and len(dc.random_cases()) == 60
    for c in dc.named_cases():
        assert c["reason"] or c["why"], c["name"]
        assert set(c["reason"]) <= set(dc.DEFECTS), c["name"]
    for c in dc.random_cases():
        K, S = c["moveouts"].shape
        assert K <= 700 and S <= 40
    # what the names promise
    shape = {c["name"]: c["moveouts"].shape for c in dc.named_cases()}
    assert shape["S1"][1] == 1 and shape["K1"][0] == 1 and shape["K2_kept"][0] == shape["K2_redundant"][0] == 2
    assert shape["S256_all"] == shape["S256_some"] == (300, 256) and shape["S80"][1] == 80
    assert (dc.named_case("S256_all")["n_diff"], dc.named_case("S256_some")["n_diff"]) == (256, 17)
    assert dc.named_case("n_diff_1")["n_diff"] == 1 and shape["chain_across_batches"][0] == 1200
    for name in ("cells_change_answer", "on_vertices", "outside_cells", "nan_coordinates", "descending_vertices",
                 "many_empty_cells"):
        c = dc.named_case(name)
        assert len(c["cell_lon"]) != len(c["cell_lat"]), name
        assert len(np.unique(np.diff(c["cell_lon"]).round(4))) > 1 and len(np.unique(np.diff(c["cell_lat"]).round(4))) > 1, name
    c = dc.named_case("many_empty_cells")
    assert (len(c["cell_lon"]) - 1, len(c["cell_lat"]) - 1) == (12, 9)
    c = dc.named_case("on_vertices")
    assert np.isin(c["lon"], c["cell_lon"]).sum() > 20 and np.isin(c["lat"], c["cell_lat"]).sum() > 20
    assert (c["lon"] == c["cell_lon"][-1]).any() and (c["lat"] == c["cell_lat"][-1]).any()
    c = dc.named_case("outside_cells")
    assert ((c["lon"] < c["cell_lon"][0]) | (c["lon"] >= c["cell_lon"][-1])).sum() > 100
    c = dc.named_case("nan_coordinates")
    assert np.isnan(c["lon"]).sum() > 10 and np.isnan(c["lat"]).sum() > 10
    c = dc.named_case("nan_moveouts")
    assert np.isnan(c["moveouts"]).all(axis=1).any() and np.isinf(c["moveouts"]).any()
    c = dc.named_case("tie_at_threshold")
    assert dc.threshold2(c["threshold"], c["n_diff"]) == 1.0 and np.array_equal(c["moveouts"] * 2, np.round(c["moveouts"] * 2))


def test_selection_sorts_are_the_references():
    assert dc.selection_argsort([1.0, 1.0, 0.0]) == [2, 1, 0]                     # swap-based: not stable
    assert list(np.argsort([1.0, 1.0, 0.0], kind="stable")) == [2, 0, 1]
    rng = np.random.default_rng(3)
    mv = rng.integers(0, 4, (50, 9)).astype(np.float32)
    mv[7, 3] = mv[9, 0] = np.nan
    rank = dc.rankings(mv)
    for k in range(50):
        assert list(rank[k]) == dc.selection_argsort(mv[k]), k


@pytest.mark.parametrize("method", dc.METHODS)
def test_definition_equals_the_oracle(oracle_lib, answers, method):
    for case in dc.named_cases() + dc.random_cases():
        want = oracle_lib.find_similar_sources(*dc.args_of(case), method)
        got = answers[case["name"], method]
        assert got.dtype == bool and np.array_equal(got, want), (case["name"], np.flatnonzero(got != want)[:8])


@pytest.mark.parametrize("method", dc.METHODS)
def test_definition_equals_the_recorded_reference(answers, recorded, method):
    cases = dc.named_cases() + dc.random_cases()
    assert len(recorded) == 2 * len(cases)
    for case in cases:
        want = _recorded_flags(recorded, case, method)
        got = answers[case["name"], method]
        assert np.array_equal(got, want), (case["name"], np.flatnonzero(got != want)[:8])


@pytest.mark.parametrize("method", dc.METHODS)
@pytest.mark.parametrize("ndiff", [5, 9])
def test_definition_equals_the_first_golden_file(method, ndiff):
    g = np.load(os.path.join(GOLD, "similar_sources.npz"))
    red = dc.definition(g["moveouts"], g["lon"], g["lat"], g["cell_lon"], g["cell_lat"],
                        float(g[f"thr_{method}_{ndiff}"]), ndiff, method)
    assert np.array_equal(red, g[f"red_{method}_{ndiff}"])


def test_every_defect_is_rejected_by_the_cases_that_name_it(answers):
    matrix = {}
    for defect in dc.DEFECTS:
        rejecting = []
        for case in dc.named_cases():
            hit = [m for m in dc.DEFECT_METHODS[defect]
                   if not np.array_equal(dc.definition(*dc.args_of(case), m, defect=defect), answers[case["name"], m])]
            if hit:
                rejecting.append(case["name"] + ("" if len(hit) == 2 else f" ({hit[0]})"))
            assert hit or defect not in case["reason"], f"{case['name']} names {defect} and does not reject it"
        matrix[defect] = rejecting
        assert any(defect in c["reason"] for c in dc.named_cases()), f"no case names {defect}"
    print("defect x named cases that reject it")
    for defect, rejecting in matrix.items():
        named = [c["name"] for c in dc.named_cases() if defect in c["reason"]]
        print(f"  {defect} ({len(rejecting)} cases; named by {', '.join(named)}):\n      " + ", ".join(rejecting))


def test_the_pairs_of_the_rounding_cases_sit_between_the_two_sums():
    """What the seeded searches claim: on the two-source cases the planted rounding alone moves the pair across thr2."""
    for name, defect, method in (("rounding_closest_f32_square", "f32_square", "closest"),
                                 ("rounding_closest_f64_acc", "f64_accumulate", "closest"),
                                 ("rounding_smallest_f64_acc", "f64_accumulate", "smallest"),
                                 ("thr2_rounding", "thr2_in_float", "closest"),
                                 ("smallest_add_order", "smallest_in_station_order", "smallest")):
        c = dc.named_case(name)
        assert c["moveouts"].shape[0] == 2 and c["reason"] == (defect,)
        good = dc.definition(*dc.args_of(c), method)
        bad = dc.definition(*dc.args_of(c), method, defect=defect)
        assert not good[0] and not bad[0] and good[1] != bad[1], name


def test_cases_are_not_trivial(answers, recorded):
    """On the reference's recorded answers alone (and so on the definition's)."""
    for case in dc.named_cases():
        shares = [_recorded_flags(recorded, case, m).mean() for m in dc.METHODS]
        if case["name"] not in dc.DEGENERATE:
            assert any(0.05 <= s <= 0.95 for s in shares), (case["name"], shares)
    flags = np.concatenate([_recorded_flags(recorded, c, m) for c in dc.random_cases() for m in dc.METHODS])
    assert flags.sum() > 10_000 and (~flags).sum() > 10_000, (flags.sum(), (~flags).sum())
    # the cell pass decides: without it the answer is another one
    c = dc.named_case("cells_change_answer")
    for m in dc.METHODS:
        assert not np.array_equal(dc.definition(*dc.args_of(c), m, defect="no_cell_pass"), answers[c["name"], m])
    # a chain alternates; one that crosses batches keeps half of 1200
    for name in ("chain_in_batch", "chain_across_batches"):
        red = answers[name, "closest"]
        assert np.array_equal(red, np.arange(len(red)) % 2 == 1), name
    assert (~answers["chain_across_batches", "smallest"]).sum() == 600 > 2 * dc.FS_BATCH
    assert not np.array_equal(answers["chain_shuffled", "closest"], answers["chain_across_batches", "closest"])
    # degenerate on purpose
    for m in dc.METHODS:
        assert not answers["thr0", m].any() and not answers["nan_threshold", m].any() and not answers["K1", m].any()
        assert answers["thr_big", m][1:].all() and not answers["thr_big", m][0]
        assert list(answers["K2_redundant", m]) == [False, True] and list(answers["K2_kept", m]) == [False, False]
        c = dc.named_case("negative_threshold")
        a = list(dc.args_of(c))
        a[5] = abs(a[5])
        assert a[5] != c["threshold"] and np.array_equal(dc.definition(*a, m), answers[c["name"], m])


def test_batch_seam_cases_meet_the_seam(answers):
    """The candidates the global pass starts with (what the cell pass left) number exactly FS_BATCH, or one more, and
    the last of them is the last source; the cell of batch_exact_in_cell holds exactly FS_BATCH members."""
    for name, n in (("batch_exact_256", dc.FS_BATCH), ("batch_257", dc.FS_BATCH + 1)):
        c = dc.named_case(name)
        for m in dc.METHODS:
            after_cells = dc.definition(*dc.args_of(c), m, global_pass=False)
            assert (~after_cells).sum() == n and not after_cells[-1], (name, (~after_cells).sum())
            assert after_cells.sum() >= 60 and (answers[name, m] & ~after_cells).sum() >= 40
        if name == "batch_257":
            assert answers[name, "closest"][-1] and not dc.definition(*dc.args_of(c), "closest", global_pass=False)[-1]
    c = dc.named_case("batch_exact_in_cell")
    inside = c["lon"] == np.float32(0.1)
    assert inside.sum() == dc.FS_BATCH and inside[-1] and 0 < (answers[c["name"], "closest"] & inside).sum() < 200
