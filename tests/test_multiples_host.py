"""CPU: the definition of the multiples flagging -- postprocess.flag_multiples, the loop of
TemplateGroup.remove_multiples (BPMF/dataset.py:5214-5282) on plain arrays -- against the reference's own answers
(tests/golden/multiples.npz, written by tests/golden/make_multiples_golden.py; and the imported reference itself where
its tree is at hand), the sharpness of the case list the GPU test shares (multiples_cases.py), and the two functions
built on it: workflow.detections_unique and the `multiples=` option of workflow.sharded_matched_filter_detections
(gloo, two ranks)."""
import importlib.util
import os
import socket
import sys
from unittest.mock import MagicMock

import numpy as np
import pytest

import multiples_cases as mc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "multiples.npz")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def mm():
    return _load("make_multiples_golden")


def test_mirror_equals_the_recorded_reference(mm):
    from seismic_bpmf_amd import postprocess as pp
    g = np.load(GOLDEN)
    n_cases = int(g["n_cases"])
    assert n_cases >= 30
    flagged, criteria = 0, set()
    for j in range(n_cases):
        case = {k: g[f"{k}_{j}"] for k in ("origin_time_ms", "event_tids", "cc", "tids", "ellipsoid_dist",
                                           "intertemplate_cc", "similarity_criterion", "distance_criterion",
                                           "dt_criterion")}
        n = len(case["cc"])
        want = np.unpackbits(g[f"unique_event_{j}"])[:n].astype(bool)
        assert n <= 400 and (~want).sum() >= 1, j
        assert len(np.unique(case["origin_time_ms"])) == n, j          # the reference is order-dependent on ties
        assert not np.array_equal(np.diff(case["tids"]), np.ones(len(case["tids"]) - 1)), j
        got = pp.flag_multiples(*mm.mirror_arguments(case, pp))
        assert got.dtype == bool and np.array_equal(got, want), j
        flagged += int((~want).sum())
        criteria.add((float(case["similarity_criterion"]), float(case["distance_criterion"]), float(case["dt_criterion"])))
    assert flagged >= 1000 and criteria == set(mm.CRITERIA)


def test_mirror_equals_the_live_reference(mm):
    """Fresh seeds, distinct times, against the reference imported with make_goldens.py's stub modules."""
    import sys
    from seismic_bpmf_amd import postprocess as pp
    mg = _load("make_goldens")
    ref = os.environ.get("BPMF_RECORD_REFERENCE") or mg.REF
    if not os.path.isdir(os.path.join(ref, "BPMF")):
        pytest.skip(f"no reference source tree at {ref} (set BPMF_RECORD_REFERENCE): the recorded answers of "
                    "tests/golden/multiples.npz are checked instead")
    mg.REF = ref
    cwd, path0, mods0 = os.getcwd(), list(sys.path), set(sys.modules)
    try:
        try:
            mg.import_reference()
            from BPMF import dataset
        finally:
            os.chdir(cwd)
        flagged = 0
        for j, case in enumerate(mm.reference_cases(seed=977, repeats=1, n_max=200)):
            want = mm.reference_unique_event(dataset, case)
            assert np.array_equal(pp.flag_multiples(*mm.mirror_arguments(case, pp)), want), j
            flagged += int((~want).sum())
        assert flagged >= 100
    finally:
        for name in set(sys.modules) - mods0:
            if isinstance(sys.modules[name], MagicMock) or name == "BPMF" or name.startswith("BPMF."):
                del sys.modules[name]
        sys.path[:] = path0


def test_restated_definition_equals_the_mirror_on_every_shared_case():
    from seismic_bpmf_amd import postprocess as pp
    for name, *args in mc.named_cases() + mc.random_cases(count=40):
        assert np.array_equal(mc.definition(*args), pp.flag_multiples(*args)), name


def test_split_triples_put_sum_and_difference_on_opposite_sides():
    for t, dt, sum_smaller in mc.split_triples():
        acc, direct = (t[1] - t[0]) + (t[2] - t[1]), t[2] - t[0]
        assert (acc < dt) != (direct < dt) and (acc < dt) == sum_smaller


@pytest.mark.parametrize("variant", mc.VARIANTS)
def test_named_cases_are_sharp(variant):
    """Each way of getting the definition wrong changes the result of at least one named case."""
    from seismic_bpmf_amd import postprocess as pp
    differs = [name for name, *args in mc.named_cases()
               if not np.array_equal(mc.definition(*args, variant=variant), pp.flag_multiples(*args))]
    assert differs, variant


def test_arguments_are_checked():
    from seismic_bpmf_amd import postprocess as pp
    ok = np.ones((2, 2), bool)
    for bad_cc in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="finite"):
            pp.flag_multiples([0.0, 1.0], [0, 1], [0.5, bad_cc], ok, 4.0)
    for rows in ([0, 2], [-1, 0]):
        with pytest.raises(ValueError, match="outside"):
            pp.flag_multiples([0.0, 1.0], rows, [0.5, 0.5], ok, 4.0)
    with pytest.raises(ValueError):
        pp.flag_multiples([0.0, 1.0], [0], [0.5, 0.5], ok, 4.0)
    with pytest.raises(ValueError):
        pp.multiples_pair_mask(np.zeros((2, 2)), 1.0, None, 0.5)
    dist, sim = np.array([[0.0, 0.5], [2.0, np.nan]]), np.array([[1.0, 0.05], [0.9, 1.0]])
    assert np.array_equal(pp.multiples_pair_mask(dist, 1.0), [[True, True], [False, False]])
    assert np.array_equal(pp.multiples_pair_mask(dist, 1.0, sim, 0.1), [[True, False], [False, False]])
    assert np.array_equal(pp.multiples_pair_mask(dist, 1.0, sim, -1.0), [[True, True], [False, False]])


def _detections(seed=5, T=5):
    rng = np.random.default_rng(seed)
    det = {}
    for t in range(T):
        idx = np.unique(rng.integers(0, 400, int(rng.integers(0, 40)))) * 10          # common samples: time ties
        det[t] = (idx.astype(np.int64), rng.random(len(idx)).astype(np.float32), np.ones(len(idx), np.float32))
    return det, rng.random((T, T)) < 0.6


def test_detections_unique_equals_the_mirror():
    from seismic_bpmf_amd import postprocess as pp, workflow
    det, ok = _detections()
    got = workflow.detections_unique(det, sr=25.0, step=2, pair_ok=ok, dt_criterion=4.0, t0_sec=86400.0, on_host=True)
    t = np.concatenate([86400.0 + det[k][0] * 2 / 25.0 for k in sorted(det)])
    rows = np.concatenate([np.full(len(det[k][0]), k) for k in sorted(det)])
    want = pp.flag_multiples(t, rows, np.concatenate([det[k][1] for k in sorted(det)]), ok, 4.0)
    assert sorted(got) == sorted(det) and (~want).sum() > 5
    assert np.array_equal(np.concatenate([got[k] for k in sorted(det)]), want)
    assert all(got[k].dtype == bool and got[k].shape == det[k][0].shape for k in det)


# ---- the sharded search with multiples=, gloo, two ranks (stand-in engine and detector: no device) ----
class _Engine:
    def __init__(self):
        import torch
        self.device = torch.device("cpu")

    def set_data(self, data):
        self.data = np.asarray(data, dtype=np.float32)

    def run(self, templates, moveouts, weights, step=1, network_sum=True):
        import torch
        return torch.zeros((np.asarray(weights).shape[0], 8))


def _detector_for(t0_holder):
    def detector(cc, moveouts, weights, *, step, sr):
        det, _ = _detections()
        first = int(np.asarray(moveouts)[0, 0, 0])                  # the moveouts carry the global template id
        return {k: det[first + k] for k in range(cc.shape[0])}
    return detector


def _inputs():
    T = 5
    moveouts = np.arange(T, dtype=np.int32).reshape(T, 1, 1) * np.ones((T, 2, 3), np.int32)
    return np.zeros((T, 2, 3, 8), np.float32), moveouts, np.ones((T, 2, 3), np.float32), np.zeros((2, 3, 64), np.float32)


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from seismic_bpmf_amd import workflow
    tp, mv, w, data = _inputs()
    _, ok = _detections()
    kw = dict(engine=_Engine(), detector=_detector_for(None), step=2, balance=False, sr=25.0)
    det, info = workflow.sharded_matched_filter_detections(tp, mv, w, data, **kw,
                                                           multiples=dict(pair_ok=ok, dt_criterion=4.0, t0_sec=7.0))
    plain, info_plain = workflow.sharded_matched_filter_detections(tp, mv, w, data, **kw)
    assert "unique_event" not in info_plain and sorted(info_plain) == sorted(k for k in info if k != "unique_event")
    assert all(np.array_equal(plain[t][j], det[t][j]) for t in det for j in range(3))
    q.put((rank, info["templates"], {t: v[0].tolist() for t, v in det.items()},
           {t: v.tolist() for t, v in info["unique_event"].items()}))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_search_flags_the_same_multiples_on_every_rank():
    import torch.multiprocessing as mp
    from seismic_bpmf_amd import postprocess as pp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = sorted((q.get(timeout=600) for _ in range(2)), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    det, ok = _detections()
    order = sorted(det)
    t = np.concatenate([7.0 + det[k][0] * 2 / 25.0 for k in order])
    want = pp.flag_multiples(t, np.concatenate([np.full(len(det[k][0]), k) for k in order]),
                             np.concatenate([det[k][1] for k in order]), ok, 4.0)
    assert (~want).sum() > 5
    assert results[0][1] != results[1][1]                           # two shards
    for rank, _, found, unique in results:
        assert all(found[k] == det[k][0].tolist() for k in order), rank
        assert np.array_equal(np.concatenate([np.asarray(unique[k], bool) for k in order]), want), rank
        assert unique == results[0][3], rank
