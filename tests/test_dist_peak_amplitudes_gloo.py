"""CPU, gloo, world sizes 2 and 4: the peak amplitudes of workflow.sharded_matched_filter_detections
(BPMF/similarity_search.py:695-714 inside the chunk loop of run_matched_filter_search, :726-807 -- the chunks are the
ranks here).  Every rank gathers the amplitudes of ITS templates' detections (a stand-in engine without a device: the
host mirror), a second all-gather of (n, S * C) rows brings them together: info["peak_amplitudes"] must be identical
on every rank, equal to the one-process result and ordered like the detections.  One rank's shard has no detection."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 50.0
AMP_KW = dict(offset_win_peak_amp_sec=0.5, duration_win_peak_amp_sec=2.0)       # 25 and 100 samples
QUIET = (4, 5, 6, 7)  # templates without a weighted channel: the last shard(s) of both world sizes hold no detection


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class OracleMF:
    """MatchedFilterGPU's interface on the CPU oracle: the day stays a host array."""
    device = torch.device("cpu")

    def set_data(self, data):
        self.data = np.ascontiguousarray(data.numpy() if isinstance(data, torch.Tensor) else data, dtype=np.float32)

    def run(self, templates, moveouts, weights, step=1, network_sum=True):
        from oracle import oracle
        return torch.from_numpy(oracle.matched_filter(np.asarray(templates), np.asarray(moveouts), np.asarray(weights),
                                                      self.data, step, network_sum, num_threads=1))


def detector(cc, moveouts, weights, *, step, sr, window, n_dev, search_win):
    """Host mirror of the reference's MAD threshold + select_cc_indexes, rows -> (idx, cc, thr)."""
    from seismic_bpmf_amd import postprocess as pp
    cc = cc.numpy() if isinstance(cc, torch.Tensor) else cc
    out = {}
    wn = np.random.default_rng(3).standard_normal(cc.shape[1]).astype(np.float32)
    for t in range(cc.shape[0]):
        row = cc[t]
        if not (row != 0).any():
            out[t] = (np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros(0, np.float32))
            continue
        thr = pp.time_dependent_threshold_mad(row, window, n_dev, overlap=0.5, white_noise=wn).astype(np.float32)
        idx = pp.select_cc_indexes(row, thr, search_win, step=step, sr=sr, data_duration_sec=0.0, n_dev_threshold=n_dev,
                                   min_freq_hz=2.0, data_buffer_sec=0.0, threshold_type="mad", remove_edges=False)
        out[t] = (idx, row[idx].astype(np.float32), thr[idx])
    return out


DET_KW = dict(sr=SR, window=600, n_dev=6.0, search_win=40)


def case():
    sys.path.insert(0, ROOT)
    from seismic_bpmf_amd import synthetic as syn
    m = syn.make_mf_inputs(T=8, S=4, C=3, L=32, N=6000, seed=31, max_moveout=60, n_events=3)
    w = m["weights"].copy()
    w[QUIET, :, :] = 0.0
    m["weights"] = w
    # the phases of the peak-amplitude windows are not those of the matched filter; a day scaled per channel
    m["moveouts_peak_amp"] = np.ascontiguousarray(m["moveouts"][:, :, ::-1]) - 7
    m["data_norm"] = np.random.default_rng(5).uniform(0.5, 4.0, (4, 3)).astype(np.float32)
    return m


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from seismic_bpmf_amd import workflow
    m = case()
    src = world - 1                              # the day lives on the last rank only
    det, info = workflow.sharded_matched_filter_detections(
        m["templates"], m["moveouts"], m["weights"], m["data"] if rank == src else None, engine=OracleMF(),
        detector=detector, data_src=src, step=1, balance=False, extract_peak_amplitudes=True,
        moveouts_peak_amp=m["moveouts_peak_amp"], data_norm=m["data_norm"], **AMP_KW, **DET_KW)
    plain, info_plain = workflow.sharded_matched_filter_detections(
        m["templates"], m["moveouts"], m["weights"], m["data"] if rank == src else None, engine=OracleMF(),
        detector=detector, data_src=src, step=1, balance=False, **DET_KW)
    assert "peak_amplitudes" not in info_plain
    assert all(np.array_equal(plain[t][0], det[t][0]) for t in det)
    q.put((rank, info["templates"], {t: v[0].tolist() for t, v in det.items()}, info["peak_amplitudes"]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_peak_amplitudes_equal_the_single_process_result(oracle_lib, world):
    sys.path.insert(0, ROOT)
    from seismic_bpmf_amd import postprocess as pp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = sorted((q.get(timeout=600) for _ in range(world)), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    # ---- one process over all templates
    m = case()
    T, S, C = m["weights"].shape
    cc = oracle_lib.matched_filter(m["templates"], m["moveouts"], m["weights"], m["data"], 1)
    want_det = detector(cc, m["moveouts"], m["weights"], step=1, **DET_KW)
    want = {t: pp.peak_amplitudes_host(m["data"], np.full(len(want_det[t][0]), t), want_det[t][0],
                                       m["moveouts_peak_amp"], 25, 100, m["data_norm"]) for t in range(T)}
    assert sum(len(v[0]) for v in want_det.values()) >= 3 * (T - len(QUIET))     # the planted events are found
    # a rank whose shard holds no detection takes part in both all-gathers
    shards = [r[1] for r in results]
    assert any(t1 > t0 and sum(len(want_det[t][0]) for t in range(t0, t1)) == 0 for t0, t1 in shards), shards
    for rank, _, det, amp in results:
        assert sorted(amp) == list(range(T)), rank
        for t in range(T):
            assert det[t] == want_det[t][0].tolist(), (rank, t)
            assert amp[t].shape == (len(det[t]), S, C) and amp[t].dtype == np.float32, (rank, t)
            assert np.array_equal(amp[t], want[t], equal_nan=True), (rank, t)     # ordered like the detections
            assert np.array_equal(amp[t], results[0][3][t], equal_nan=True), (rank, t)
    assert all(want[t].shape[0] > 0 and (want[t] != 0).all() for t in range(T) if t not in QUIET)
