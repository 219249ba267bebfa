"""CPU: the schedule of a backprojection run (bpmf_bp_launch_info = bp_plan_host + bp_schedule of csrc/bp_plan.hip).

Which path a run takes, how many group ranges per tile, where the interior range starts and ends and where the
partial rows lie decide which samples are written at all: a slip here shows on a GPU only, as samples nobody wrote
(round 4: the last partial tile, with every used moveout negative).  Here the schedule is restated in Python,
independently of the C++ -- written from bp_run_dev, bp_workspace_bytes, bp_max_batch, dispatch_beam and
bpmf_bp_plan_info as they stood before the schedule became one function -- and compared with the library field by
field on every boundary; the fields of the plan's shape are taken as the info call reports them.  Properties that
hold whatever the restatement says are asserted on every case as well, and the facts of the shape that can be
derived by hand are asserted on tiny tables.  Nothing here needs a device."""
import numpy as np
import pytest

from seismic_bpmf_amd import _lib

DEFAULTS = {"bp.split": -1, "bp.dual": 1, "bp.fast": 1, "bp.tpt": 2, "bp.direct": 0, "bp.halves": 1, "bp.fast_tile": 0,
            "bp.max_group": 4096, "bp.compat_strict_upper_only": 0}


def align_up(x, a):
    return (x + a - 1) // a * a


def trunc_div(a, b):
    """C++ integer division (towards zero)."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


# ------------------------------------------------------------------ the restatement ---
def expected_kernel(sh):
    """dispatch_beam's switch and the waves_per_cu / gather_bytes / tile lines of bpmf_bp_plan_info."""
    k = dict(family=None, wpb=0, nsv=0, b64=False, ntv=0, tpt=0, nblk=0, tile=0, lds_bytes=0, waves_per_cu=8,
             gather_bytes=8 if sh["dual"] else 4)
    if sh["direct"]:
        k.update(tile=1024, gather_bytes=4)
        return k
    if sh["tpt"] == 2 and sh["nsv"] in (4, 8, 12, 16, 32):
        wpb, b64 = (16, False) if sh["nsv"] == 32 else ((16, True) if sh["dual"] else (12, False))
        k.update(family="wps2", wpb=wpb, nsv=sh["nsv"], b64=b64, tile=512, lds_bytes=max(sh["lds_bytes"], 2 * wpb * 512 * 4),
                 waves_per_cu=16 if sh["nsv"] > 16 else (16 if sh["dual"] else 24))
    elif sh["tpt"] == 2 and sh["ntv"] in (8, 16, 24, 32):
        k.update(family="wps", ntv=sh["ntv"], tile=512, lds_bytes=max(sh["lds_bytes"], 8 * 512 * 4))
    else:
        tpt = 1 if sh["tpt"] == 1 else 2
        k.update(family="readlane", tpt=tpt, nblk=1 if sh["NT"] <= 64 else (2 if sh["NT"] <= 128 else 4), tile=256 * tpt,
                 lds_bytes=sh["lds_bytes"])
    return k


def split_wanted(N, forced, n_events=1):
    n_tiles = (N + 511) // 512 * n_events
    want = 1 if n_tiles >= 1024 else (1024 + n_tiles - 1) // n_tiles
    if forced >= 0:
        want = 1 if forced < 1 else forced
    return want


def generic_can_split(sh):
    return sh["tpt"] == 2 and sh["nsv"] != 0 and sh["n_groups"] >= 2


def bp_split_count(sh, N, forced, n_events=1):
    if not generic_can_split(sh):
        return 1
    return max(1, min(split_wanted(N, forced, n_events), sh["n_groups"]))


def bp_fast_split_counts(sh, N, forced):
    want = split_wanted(N, forced)
    for c in sh["classes"]:
        want = min(want, c["n_groups"] // c["n_pass"])
    if generic_can_split(sh):
        want = min(want, sh["n_groups"])
    n_split = max(1, want)
    return n_split, (n_split if generic_can_split(sh) else 1)


def direct_split_count(sh, N):
    tiles = (N + 1023) // 1024
    want = 1 if tiles >= 1024 else (1024 + tiles - 1) // tiles
    return max(1, min(want, sh["K"], 256))


def expected_schedule(sh, N, reduce, forced, n_events):
    is_max = reduce == "max"
    prestack = align_up(sh["S"] * sh["P"] * N * 4, 256)
    s = dict(kernel=expected_kernel(sh), lo_s=0, hi_s=0, o_prestack=0)
    if n_events:                    # bp_max_batch / bp_max_batch_part_bytes
        E = n_events
        prestack = align_up(E * sh["S"] * sh["P"] * N * 4, 256)
        if sh["direct"]:
            rows = direct_split_count(sh, N)
            s.update(path="direct", n_split=rows, n_split_edge=rows, rows=rows)
            part = align_up(rows * N * 8, 256) if rows > 1 else 0
            parg = prestack + rows * N * 4
        else:
            rows = bp_split_count(sh, N, forced, E)
            s.update(path="general", n_split=rows, n_split_edge=rows, rows=rows)
            part = align_up(E * rows * N * 8, 256) if rows > 1 else 0
            parg = prestack + E * rows * N * 4
        s.update(o_pbeam=prestack, o_parg=parg if rows > 1 else prestack, total=prestack + part)
        return s
    # bp_workspace_bytes
    ws_rows = direct_split_count(sh, N) if sh["direct"] else bp_split_count(sh, N, forced)
    if sh["fast"]:
        ws_rows = max(ws_rows, bp_fast_split_counts(sh, N, forced)[0] * sh["n_classes"])
    total = prestack + (align_up(ws_rows * N * 8, 256) if ws_rows > 1 else 0)
    # bp_run_dev
    if sh["direct"]:
        rows = direct_split_count(sh, N) if is_max else 1
        s.update(path="direct", n_split=rows, n_split_edge=rows, rows=rows)
    elif sh["fast"] and is_max:
        n_split, n_split_edge = bp_fast_split_counts(sh, N, forced)
        rows = n_split * sh["n_classes"]
        lo_s = (-sh["tmin_all"] + 1023) // 1024 * 1024 if sh["tmin_all"] < 0 else 0
        hi_s = trunc_div(N - sh["tmax_all"] - 8, 1024) * 1024
        if N - sh["tmax_all"] - 8 < 0:
            hi_s = 0
        hi_s = min(hi_s, N // 1024 * 1024)
        lo_s = min(lo_s, N)
        hi_s = max(lo_s, hi_s)
        s.update(path="interior + edges", n_split=n_split, n_split_edge=n_split_edge, rows=rows, lo_s=lo_s, hi_s=hi_s)
    else:
        n_split = bp_split_count(sh, N, forced)
        rows = n_split if is_max else 1
        s.update(path="general", n_split=n_split, n_split_edge=n_split, rows=rows)
    s.update(o_pbeam=prestack, o_parg=prestack + rows * N * 4 if rows > 1 else prestack, total=total)
    return s


def expected_plan_info(sh):
    k = expected_kernel(sh)
    z = [0, 0, 0]
    if sh["direct"]:
        return dict(n_groups=0, tile=1024, lds_bytes=0, gather_bytes=4, stations_max=0, waves_per_cu=8, n_classes=0,
                    class_tile=z, class_sources=z, class_groups=z, class_stations_max=z)
    info = dict(n_groups=sh["n_groups"], tile=256 * sh["tpt"], lds_bytes=sh["lds_bytes"], gather_bytes=k["gather_bytes"],
                stations_max=sh["nsv"], waves_per_cu=k["waves_per_cu"], n_classes=sh["n_classes"])
    cl = sh["classes"]
    pad = lambda name: [c[name] for c in cl] + [0] * (3 - len(cl))
    info.update(class_tile=pad("tile"), class_sources=pad("n_sources"), class_groups=pad("n_groups"),
                class_stations_max=pad("max_stations"))
    if sh["fast"]:
        big = 0
        for c in range(1, len(cl)):
            if cl[c]["n_sources"] > cl[big]["n_sources"]:
                big = c
        info.update(tile=cl[big]["tile"], n_groups=cl[big]["n_groups"], lds_bytes=cl[big]["lds_bytes"], gather_bytes=8,
                    waves_per_cu=16)
    return info


# ------------------------------------------------------------------------- tables ---
def table(K=24, S=8, P=2, used=8, lo=0, hi=300, seed=0, no_station=()):
    """(K, S, P) moveouts in [lo, hi] -- both extremes on a used station -- and (K, S) weights with `used` stations
    per source (an int, or one count per source); sources in `no_station` have none."""
    rng = np.random.default_rng(seed)
    mv = rng.integers(lo, hi + 1, size=(K, S, P)).astype(np.int32)
    ws = np.zeros((K, S), np.float32)
    counts = [used] * K if np.isscalar(used) else list(used)
    for k in range(K):
        if k not in no_station:
            ws[k, rng.permutation(S)[:counts[k]]] = 1.0 + 0.25 * (k % 3)
    k0 = next(k for k in range(K) if k not in no_station)
    on = np.flatnonzero(ws[k0])
    mv[k0, on[0], 0] = lo
    mv[k0, on[-1], P - 1] = hi           # (one station and one phase: the upper extreme only)
    return mv, ws


TABLES = {
    "plain": dict(),                                                 # tmax_all = 300
    "signed": dict(lo=-100, hi=200),                                 # lo_s rounded up
    "signed_far": dict(lo=-1500, hi=200),
    "negative": dict(lo=-3000, hi=-20),                              # every used moveout negative, tmax_all < -8
    "groups": dict(K=40),
    "many": dict(K=300, S=4, used=3),                                # more sources than source ranges of bp_direct.hip                                            # with bp.max_group = 4: 10 groups
    "two_classes": dict(K=40, S=24, used=[10, 20] * 20),
    "halves": dict(K=40, S=44, used=40),                             # 33-64 stations: the multi-residency class
}
for n in (3, 7, 11, 15, 20):
    TABLES[f"sta{n}"] = dict(K=12, S=n + 1, used=n, hi=40)      # (few rows, short windows: one group at tile 512)
TABLES["sta40"] = dict(K=12, S=44, used=40, hi=40)
for n in (8, 16, 24, 32, 33, 64, 65, 128, 129):
    TABLES[f"p1_{n}"] = dict(K=12, S=max(n, 8), P=1, used=n, hi=40)
for n in (2, 3, 5, 6, 8, 10, 11, 21, 22, 42, 43):                    # 3 n terms, padded to 4: both sides of 8 .. 128
    TABLES[f"p3_{n}"] = dict(K=12, S=max(n, 8), P=3, used=n, hi=40)
_cache = {}


def get_table(name):
    if name not in _cache:
        _cache[name] = table(**TABLES[name])
    return _cache[name]


def case(tab="plain", N=5000, reduce="max", n_events=0, **opts):
    return dict(tab=tab, N=N, reduce=reduce, n_events=n_events, **opts)


CASES = []
# N at and around 1024, 2048 and tmax_all + 8 = 308 (the first N with a non-negative interior bound); no interior; 1
CASES += [case(N=N, reduce=r) for N in (1, 100, 307, 308, 309, 1023, 1024, 1025, 1331, 1332, 1333, 2047, 2048, 2049,
                                         2355, 2356, 2357, 5000) for r in ("max", "none")]
# tmin_all < 0: lo_s rounded up to 1024 / 2048, also beyond N
CASES += [case("signed", N=N) for N in (1, 99, 100, 101, 1023, 1024, 1025, 1231, 1232, 1233, 2048, 5000)]
CASES += [case("signed_far", N=N) for N in (700, 1499, 1500, 2047, 2048, 2049, 2255, 2256, 2257, 5000)]
# every used moveout negative, tmax_all = -20 < -8: N - tmax_all - 8 exceeds N (the round-4 case)
CASES += [case("negative", N=N) for N in (1, 700, 1023, 1024, 1025, 2999, 3000, 3001, 3071, 3072, 3073, 4095, 4096, 4097,
                                          5000)]
# group ranges per tile: tile counts 1, 2, 1023, 1024; bp.split; the limit by n_groups (bp.max_group = 4: 10 groups)
TILE_N = (1, 512, 513, 1024, 512 * 1023 - 1, 512 * 1023, 512 * 1023 + 1, 512 * 1024 - 1, 512 * 1024, 512 * 1024 + 1)
CASES += [case("groups", N=N, reduce=r, bp__max_group=4) for N in TILE_N for r in ("max", "none")]
CASES += [case("groups", N=N, bp__max_group=g) for N in (700, 3000, 60000, 200000) for g in (1, 4, 4096)]
CASES += [case("groups", N=N, reduce=r, bp__max_group=4, bp__split=s) for N in (700, 5000, 512 * 1024)
          for s in (-1, 0, 1, 3, 10, 11, 10000) for r in ("max", "none")]
CASES += [case("groups", N=N, bp__max_group=4, bp__split=s, bp__fast=0) for N in (700, 5000) for s in (-1, 0, 3, 10000)]
CASES += [case("groups", N=N, bp__max_group=4, bp__split=s, bp__dual=0) for N in (700, 5000) for s in (-1, 3)]
# ... by the groups of sources of a class: two classes, and a multi-residency class (n_groups / n_pass)
CASES += [case("two_classes", N=N, bp__max_group=g, bp__split=s) for N in (700, 3000, 5000) for g in (3, 4096)
          for s in (-1, 3)]
CASES += [case("halves", N=N, bp__max_group=g, bp__split=s, bp__fast_tile=t) for N in (700, 3000) for g in (5, 4096)
          for s in (-1, 3) for t in (0, 256)]
# batches of events: the tiles of the whole batch count
CASES += [case(t, N=N, n_events=E, bp__max_group=4, bp__split=s) for t in ("groups", "signed") for N in (700, 3000, 5000)
          for E in (1, 7, 300) for s in (-1, 3)]
CASES += [case("two_classes", N=3000, n_events=E) for E in (1, 7)]
# the plans without LDS windows: source ranges, limited by K and 256
CASES += [case(t, N=N, reduce=r, n_events=E, bp__direct=1) for t in ("plain", "groups", "many")
          for N in (1, 1024, 1025, 3000, 100000, 2 ** 20 - 1023, 2 ** 20 - 1024, 2 ** 20)
          for r, E in (("max", 0), ("none", 0), ("max", 1), ("max", 7))]
# kernel choice: packed records of 4 / 8 / 12 / 16 / 32 stations with and without dual windows
CASES += [case(f"sta{n}", N=N, reduce=r, bp__dual=d) for n in (3, 7, 11, 15, 20) for d in (0, 1) for N in (700, 5000)
          for r in ("max", "none")]
# P = 2 beyond 32 stations without the class kernels; P = 1 and P = 3 at 8 .. 129 terms; bp.tpt = 1
CASES += [case("sta40", N=N, reduce=r, bp__fast=f) for N in (700, 5000) for r in ("max", "none") for f in (0, 1)]
CASES += [case(t, N=N, reduce=r) for t in TABLES if t.startswith(("p1_", "p3_")) for N in (700, 5000) for r in ("max", "none")]
CASES += [case(t, N=3000, reduce=r, bp__tpt=1) for t in ("plain", "sta20", "p1_16", "p1_65", "p3_43", "p1_129") for r in ("max", "none")]
CASES += [case(t, N=3000, n_events=7) for t in ("p1_16", "p3_22", "sta20")]


def case_id(c):
    return "-".join(f"{k.replace('bp__', '')}={v}" for k, v in c.items())


def run_case(hip_opts, c):
    opts = {k.replace("__", "."): v for k, v in c.items() if "__" in k}
    for k, v in opts.items():
        hip_opts(k, v)
    mv, ws = get_table(c["tab"])
    got = _lib.bp_launch_info(mv, ws, c["N"], c["reduce"], c["n_events"])
    for k in opts:
        hip_opts.reset(k)
    return got, dict(DEFAULTS, **opts)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_schedule_equals_its_restatement(hip_opts, c):
    got, opts = run_case(hip_opts, c)
    sh, N = got["shape"], c["N"]
    want = expected_schedule(sh, N, c["reduce"], opts["bp.split"], c["n_events"])
    assert sorted(got["schedule"]) == sorted(want)
    for name in want:
        assert got["schedule"][name] == want[name], (name, got["schedule"], want)
    assert got["plan_info"] == expected_plan_info(sh)
    # ---- whatever the restatement says ----
    s = got["schedule"]
    lo_s, hi_s = s["lo_s"], s["hi_s"]
    assert 0 <= lo_s <= hi_s <= N                                    # [0, lo_s) + [lo_s, hi_s) + [hi_s, N) = [0, N)
    assert hi_s == lo_s or (lo_s % 1024 == 0 and hi_s % 1024 == 0)
    for cl in sh["classes"]:
        assert hi_s == lo_s or (lo_s % cl["tile"] == 0 and hi_s % cl["tile"] == 0)
    if s["path"] == "interior + edges" and hi_s > lo_s:              # no source leaves the trace on an interior sample
        assert lo_s + sh["tmin_all"] >= 0 and hi_s - 1 + sh["tmax_all"] + 8 < N
    else:
        assert s["path"] == "interior + edges" or (lo_s, hi_s) == (0, 0)
    E = max(c["n_events"], 1)
    prestack = E * sh["S"] * sh["P"] * N * 4
    row_sets = 1 if s["path"] == "direct" else E
    assert s["o_prestack"] == 0 and s["o_prestack"] + prestack <= s["o_pbeam"]
    assert s["o_prestack"] % 256 == 0 and s["o_pbeam"] % 256 == 0
    assert s["rows"] >= 1 and s["n_split"] >= 1 and s["n_split_edge"] >= 1
    if s["rows"] > 1:
        # the partial beam rows, then the partial arg rows (one float / int32 array behind the other, as the
        # workspace has always held them: the arg rows start at a multiple of 4 bytes, not of 256), then the end
        assert s["o_pbeam"] + row_sets * s["rows"] * N * 4 <= s["o_parg"] and s["o_parg"] % 4 == 0
        assert s["o_parg"] + row_sets * s["rows"] * N * 4 <= s["total"]
        assert prestack + s["rows"] * N * 8 <= s["total"]
    else:
        assert prestack <= s["total"]
    if c["reduce"] == "none":
        assert s["rows"] == 1 and s["path"] != "interior + edges"
    if c["n_events"] == 0:                                           # one size serves both reduce codes
        other = run_case(hip_opts, dict(c, reduce="none" if c["reduce"] == "max" else "max"))[0]
        assert other["schedule"]["total"] == s["total"] and other["shape"] == sh


def test_cases_reach_every_answer(hip_opts):
    """The cases above are on both sides of every rule: each path, each compiled general kernel, splits limited by
    every limit, interior ranges that are empty, rounded up at the start and cut at the end."""
    seen = [(c, run_case(hip_opts, c)[0]) for c in CASES]
    sched = [g["schedule"] for _, g in seen]
    assert {s["path"] for s in sched} == set(_lib.BP_PATHS)
    kern = {tuple(s["kernel"][n] for n in ("family", "wpb", "nsv", "b64", "ntv", "tpt", "nblk")) for s in sched}
    assert kern == ({("wps2", 16, n, True, 0, 0, 0) for n in (4, 8, 12, 16)} | {("wps2", 12, n, False, 0, 0, 0) for n in (4, 8, 12, 16)} |
                    {("wps2", 16, 32, False, 0, 0, 0)} | {("wps", 0, 0, False, n, 0, 0) for n in (8, 16, 24, 32)} |
                    {("readlane", 0, 0, False, 0, t, b) for t in (1, 2) for b in (1, 2, 4)} - {("readlane", 0, 0, False, 0, 2, 4)} |
                    {(None, 0, 0, False, 0, 0, 0)})
    # (more than 128 terms at tile 512 are more than 256 KB of windows: no plan reaches bp_beam_kernel<2, 4, 4>)
    assert {s["kernel"]["waves_per_cu"] for s in sched} == {8, 16, 24}
    inter = [(g["shape"], g["schedule"]) for _, g in seen if g["schedule"]["path"] == "interior + edges"]
    assert any(s["lo_s"] == s["hi_s"] for _, s in inter) and any(s["lo_s"] == 1024 for _, s in inter)
    assert any(s["lo_s"] == 2048 for _, s in inter) and any(sh["tmax_all"] < -8 and s["hi_s"] > s["lo_s"] for sh, s in inter)
    assert any(s["n_split"] > s["n_split_edge"] for _, s in inter) and any(s["n_split_edge"] > 1 for _, s in inter)
    assert any(len(sh["classes"]) == 2 and s["rows"] == 2 * s["n_split"] > 2 for sh, s in inter)
    assert any(cl["halves"] and cl["n_pass"] > 1 and s["n_split"] == cl["n_groups"] // cl["n_pass"] > 1
               for sh, s in inter for cl in sh["classes"])
    general = [g["schedule"] for _, g in seen if g["schedule"]["path"] == "general"]
    assert {1, 3, 10} <= {s["n_split"] for s in general} and any(s["n_split"] > s["rows"] for s in general)
    direct = [g["schedule"] for _, g in seen if g["schedule"]["path"] == "direct"]
    assert {1, 11, 24, 40, 256} <= {s["rows"] for s in direct}       # by the tiles, by K, by 256


def test_restated_defaults_are_the_library_s():
    for name, value in DEFAULTS.items():
        assert _lib.get_option(name) == (value, value), name


# --------------------------------------------- the shape of the plan, derived by hand ---
def shape_of(mv, ws, N=3000):
    return _lib.bp_launch_info(mv, ws, N)["shape"]


def test_reasons_for_the_direct_path(hip_opts):
    # More than 256 terms per source: no LDS plan.  (A window is at least 256 samples, 1 KB: a source's own windows
    # exceed the 160 KB of LDS from 157 terms on, and that reason is tested first -- either one is the direct path.)
    mv, ws = table(K=10, S=70, P=4, used=65, hi=40)                  # 260 terms
    sh = shape_of(mv, ws)
    assert sh["direct"] in ("more than 256 terms per source", "windows exceed the LDS")
    assert (sh["tpt"], sh["NT"], sh["n_groups"], sh["nsv"], sh["ntv"], sh["fast"], sh["n_classes"]) == (4, 280, 0, 0, 0, False, 0)
    assert shape_of(*table(K=10, S=70, P=3, used=70, hi=4))["direct"] == "windows exceed the LDS"     # 210 x 260 x 4 B
    mv, ws = table(K=10, S=70, P=3, used=45, hi=4)                   # 135 terms of 260 samples: 140 KB at tile 256
    sh = shape_of(mv, ws)
    assert (sh["direct"], sh["NT"], sh["tpt"], sh["tmax_all"]) == (None, 136, 1, 4)
    mv, ws = get_table("plain")
    assert shape_of(mv, ws)["direct"] is None
    hip_opts("bp.direct", 1)
    assert shape_of(mv, ws)["direct"] == "bp.direct"
    hip_opts.reset("bp.direct")
    hip_opts("bp.compat_strict_upper_only", 1)
    assert shape_of(mv, ws)["direct"] is None                        # no negative used moveout: the default's plan
    mv2, ws2 = (x.copy() for x in table(K=20, S=8, used=5))
    assert shape_of(mv2, ws2)["direct"] is None
    k, s = np.argwhere(ws2 == 0)[0]
    mv2[k, s, 0] = -5                                                # negative, on a station without weight: not used
    assert shape_of(mv2, ws2)["direct"] is None
    k, s = np.argwhere(ws2 != 0)[0]
    mv2[k, s, 0] = -5
    sh = shape_of(mv2, ws2)
    assert sh["direct"] == "bp.compat_strict_upper_only with a negative used moveout" and sh["tmin_all"] == -5
    hip_opts.reset("bp.compat_strict_upper_only")
    assert shape_of(mv2, ws2)["direct"] is None


def test_extreme_moveouts_are_those_of_weighted_stations():
    mv, ws = table(K=6, S=5, P=2, used=3, lo=-7, hi=90)
    used = np.repeat(ws[:, :, None] != 0, 2, axis=2)
    mv[~used] = 100000
    sh = shape_of(mv, ws)
    assert (sh["tmin_all"], sh["tmax_all"]) == (-7, 90) and (sh["K"], sh["S"], sh["P"], sh["id_offset"]) == (6, 5, 2, 0)


def test_classes_by_station_count_and_the_shared_plan(hip_opts):
    K = 30
    # (18 stations with moveouts 0..8: 36 dual windows of 520 samples, 150 KB -- one group at every tile, which the
    # largest tile amortises best)
    # the densest source has 16 stations: one class at tile 512, which lists every source and doubles as the general plan
    mv, ws = table(K=K, S=18, hi=8, used=[16] + [9] * (K - 1))
    sh = shape_of(mv, ws)
    assert [(c["tile"], c["n_sources"], c["max_stations"], c["halves"], c["n_pass"]) for c in sh["classes"]] == [(512, K, 16, False, 1)]
    assert sh["fast"] and sh["fast_shares_generic"] and sh["dual"] and (sh["tpt"], sh["NT"], sh["nsv"]) == (2, 32, 16)
    assert sh["n_groups"] == sh["classes"][0]["n_groups"] and sh["lds_bytes"] == sh["classes"][0]["lds_bytes"]
    # a source without stations rides in that class (the shared plan lists every source; it is no source of the class)
    mv, ws = table(K=K, S=18, hi=8, used=[16] + [9] * (K - 1), no_station=(5,))
    sh = shape_of(mv, ws)
    assert [(c["tile"], c["n_sources"]) for c in sh["classes"]] == [(512, K - 1)]
    assert sh["fast_shares_generic"] and sh["dual"]
    # one source with 17 stations: two classes, the general kernels get their own plan of single windows
    mv, ws = table(K=K, S=18, hi=8, used=[17] + [9] * (K - 1))
    sh = shape_of(mv, ws)
    # (max_stations counts the padded terms of a source: 4 terms = 2 stations at a time)
    assert [(c["n_sources"], c["max_stations"]) for c in sh["classes"]] == [(K - 1, 10), (1, 18)]
    assert sh["classes"][0]["tile"] == 512 and sh["classes"][1]["tile"] in (256, 128)
    assert sh["fast"] and not sh["fast_shares_generic"] and not sh["dual"] and (sh["NT"], sh["nsv"]) == (36, 32)
    # ... and a source without stations is then in no class
    mv, ws = table(K=K, S=18, hi=8, used=[17] + [9] * (K - 1), no_station=(5,))
    sh = shape_of(mv, ws)
    assert [c["n_sources"] for c in sh["classes"]] == [K - 2, 1] and not sh["fast_shares_generic"]
    # one class that is not at tile 512 is not shared either
    mv, ws = table(K=K, S=18, hi=8, used=9)
    hip_opts("bp.fast_tile", 256)
    sh = shape_of(mv, ws)
    assert [(c["tile"], c["n_sources"]) for c in sh["classes"]] == [(256, K)]
    assert sh["fast"] and not sh["fast_shares_generic"] and not sh["dual"]
    hip_opts.reset("bp.fast_tile")
    # bp.fast = 0: the shared dual plan stays the general kernels', no class runs
    hip_opts("bp.fast", 0)
    sh = shape_of(mv, ws)
    assert sh["dual"] and not sh["fast"] and sh["classes"] == [] and not sh["fast_shares_generic"]
    hip_opts.reset("bp.fast")
    # bp.dual = 0, three phases, more than 64 stations: no classes
    hip_opts("bp.dual", 0)
    assert shape_of(mv, ws)["classes"] == []
    hip_opts.reset("bp.dual")
    assert shape_of(*table(K=K, S=18, P=3, hi=8, used=9))["classes"] == []
    assert shape_of(*table(K=8, S=70, P=2, used=65, hi=4))["classes"] == []


def test_info_checks_its_arguments():
    mv, ws = get_table("plain")
    with pytest.raises(_lib.BpmfHipError, match="bad N"):
        _lib.bp_launch_info(mv, ws, 0)
    with pytest.raises(_lib.BpmfHipError, match="bad N"):
        _lib.bp_launch_info(mv, ws, 3000, "none", 7)
    with pytest.raises(_lib.BpmfHipError, match="bad argument"):
        _lib.bp_launch_info(mv[:0], ws[:0], 3000)
