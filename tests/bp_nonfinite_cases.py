"""Non-finite features in the backprojection: the written rule, the cases and the checkers (TEST INFRASTRUCTURE, pure
NumPy; shared by tests/test_bp_nonfinite_host.py on the CPU and tests/test_gpu_bp_nonfinite.py on the device).

A NaN-filled gap, a dead channel exported as NaN and a clipped +-Inf are ordinary input.  DESIGN.md s4 "Non-finite
features" states what they may cost a beam; this module is that statement in NumPy.  The authority is the documented
scan of oracle/bpmf_oracle.c:bp_cpu plus IEEE arithmetic (the reference's own beam loop is not in its tree).

THE RULE.  U[s,p,t] the prestack (an fmaf chain over the components), b_k(t) the beam (an fmaf chain over the used terms):

1. PRESTACK.  U[s,p,t] is non-finite exactly as IEEE makes it: a NaN component gives NaN even under a zero phase weight,
   0 * +-Inf = NaN, +Inf and -Inf in one sum give NaN.
2. BEAM.  A station with beta == 0 is skipped: its bad samples cost nothing.  A flexible term outside [0, N) is dropped.
   A strict beam that is not computed is exactly +0 under reduce="none" and no candidate under "max", whatever its terms
   would have read.  Otherwise the class of b_k(t) -- finite, NaN, +Inf, -Inf -- is the class of the float64 evaluation
   of the same sum (f64_anchor.bp_f64 under np.errstate(all="ignore")), and a finite beam has the bits of the same call on
   the CLEANED features (every non-finite sample replaced by 0).  Premise: no finite partial sum overflows float32; the
   cases keep |f| within a few 10^3 and the weights within 2.
3. MAXIMUM.  A NaN beam is never the maximum; +Inf is, and several +Inf go to the lowest source index.
   default scan            (0, source id_offset) where no computed non-NaN beam is > 0: -Inf never beats the floor;
   bp.compat_first_computed the maximum over the computed non-NaN beams of any sign; (0, id_offset) where there is none
                           or where that maximum is -Inf.
   The max-beam is never NaN.
4. RELOCATION.  The focus follows rule 3 on the max-beams (postprocess.focus_from_max); the column at the focus time
   follows rule 2; the likelihood is postprocess.likelihood of that column bit for bit, NaNs at the same places: a NaN
   in the column makes the whole row NaN, an Inf maximum gives 0 on the finite entries and NaN at the Inf.  The
   reference's np.argmax over a volume that holds a NaN (the first NaN wins) is deliberately not followed.

CONDITIONS of every case, asserted from the definition alone (Refs.require): at least 20 % of the computed beams finite;
at least 100 computed beams in each of NaN, +Inf, -Inf; at least 100 samples whose every computed beam is NaN; at least
20 samples with a tied +Inf maximum where K >= 100.
"""
import functools

import numpy as np

import f64_anchor as fa

NAN, PINF, NINF = np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)
FINITE, C_NAN, C_PINF, C_NINF = range(4)
CLASS_NAMES = ("finite", "NaN", "+Inf", "-Inf")
SEAM_MULTIPLES = (1, 2, 4, 8, 16, 32)      # 128 m: the seams of tiles 128 / 256 / 512 / 1024 and of the interior / edge launches
MIN_FINITE_SHARE, MIN_PER_CLASS, MIN_ALL_NAN, MIN_TIED_INF, TIED_FROM_K = 0.20, 100, 100, 20, 100

# name -> arguments of f64_anchor.bp_case, and whether a NaN-filled station is planted (not where nearly every source uses
# every station: nothing finite would be left)
SHAPES = {
    "fast uniform": (dict(K=480, S=18, P=2, N=6000, tau_lo=-40, tau_hi=160, n_used=10, uniform=True), True),
    "fast per-station": (dict(K=480, S=18, P=2, N=6000, tau_lo=-40, tau_hi=160, n_used=10, uniform=False), True),
    "multi-residency": (dict(K=300, S=44, P=2, N=5000, tau_lo=-50, tau_hi=150, n_used=40, uniform=True), False),
    "wide moveouts": (dict(K=120, S=9, P=3, N=8000, tau_lo=-700, tau_hi=1200), False),
    "no-LDS grid": (dict(K=32, S=150, P=2, N=5000, tau_lo=-100, tau_hi=200), True),
    "default": (dict(K=200, S=8, P=2, N=3000, tau_lo=-120, tau_hi=260, n_used=5), True),
    "two stations": (dict(K=60, S=2, P=1, N=2500, tau_lo=-300, tau_hi=500), False),
    "relocation": (dict(K=300, S=12, P=2, N=2500, tau_lo=-60, tau_hi=240, n_used=7), True),
}
REGIMES = ("signed", "int")


# ---------------------------------------------------------------------------------------------- planting ---
def seam_positions(N):
    pos = [0, 1, N - 2, N - 1]
    for m in SEAM_MULTIPLES:
        pos += [i for i in (128 * m - 1, 128 * m, 128 * m + 1) if 1 < i < N - 2]
    return pos


def plant(f, tau, ws, tau_lo, tau_hi, dead_station, wp):
    """The planted copy of a case of f64_anchor.bp_case: (features, phase weights).
    * isolated bad samples at seam_positions(N), one component of a station each, cycling NaN, +Inf, -Inf over stations
      and components -- on max(1, S // 8, ceil(120 / K)) stations per position, so that a position reaches a hundred beams
      where a source spreads over many stations or the grid is small;
    * the one at sample 128 (in front of the gap at every N) is a NaN on a component whose phase weights are set to 0 (rule 1);
    * a +Inf and a -Inf on two used stations of source 5, signed so that they meet as +Inf - Inf in its beam at 3N/4;
    * a -Inf beam alone at the last sample strict bounds compute (the latest term of the source computed last reads
      sample N - 1);
    * a NaN gap over every station, tau_hi - tau_lo + 110 samples from N/8: whole samples where every beam is NaN;
    * dead_station: station S - 1 filled with NaN."""
    f0 = np.asarray(f, dtype=np.float32)
    f, wp = np.array(f, dtype=np.float32), np.array(wp, dtype=np.float32)
    S, C, N = f.shape
    live = S - 1 if dead_station else S                    # the isolated samples keep off the dead station
    values = (NAN, PINF, NINF)
    for j, i in enumerate(seam_positions(N)):
        for q in range(min(live, max(1, S // 8, -(-120 // tau.shape[0])))):     # (see the docstring)
            s = (j + (8 if live > 8 else 1) * q) % live
            c = (j // live + j + q) % C
            v = values[(j + q) % 3]
            if i == 128 and q == 0:
                v = NAN
                wp[s, c, :] = 0.0
            f[s, c, i] = v
    t_star = 3 * N // 4
    used = [s for s in np.flatnonzero(ws[5] != 0) if s < live][:2]
    assert len(used) == 2, "source 5 needs two used stations"
    for s, want in zip(used, (1.0, -1.0)):
        c = int(np.argmax(wp[s, :, 0] != 0))
        assert wp[s, c, 0] != 0, "a component with a phase weight"
        i = t_star + int(tau[5, s, 0])
        assert 0 <= i < N
        f[s, c, i] = PINF if want * wp[s, c, 0] > 0 else NINF
    # the source that strict bounds compute last, alone at its last sample: its latest term reads -Inf at N - 1, so the
    # only candidate there is -Inf (the floor under either scan)
    ok = (ws != 0).any(axis=1) & ((ws[:, live:] == 0).all(axis=1))
    hi = np.where((ws != 0)[:, :, None], tau, np.iinfo(np.int32).min).max(axis=(1, 2))
    k_last = int(np.argmin(np.where(ok, hi, np.iinfo(np.int32).max)))
    s, p = (int(x) for x in np.argwhere((tau[k_last] == hi[k_last]) & (ws[k_last] != 0)[:, None])[0])
    c = int(np.argmax(wp[s, :, p] != 0))
    f[s, :, N - 1] = f0[s, :, N - 1]
    f[s, c, N - 1] = NINF if wp[s, c, p] > 0 else PINF
    g0 = N // 8
    f[:, :, g0:g0 + (tau_hi - tau_lo + 110)] = NAN
    if dead_station:
        f[S - 1] = NAN
    return f, wp


class Case:
    """name, regime, args = (features, moveouts, phase weights, source weights) planted, clean = the same with every
    non-finite sample replaced by +0 (the planted zero phase weights stay), kw: the arguments of bp_case."""


@functools.lru_cache(maxsize=None)
def case(shape, regime, seed=0):
    kw, dead = SHAPES[shape]
    f0, tau, wp0, ws = fa.bp_case(regime, seed=7000 + 13 * len(shape) + kw["K"] + seed, **kw)
    f, wp = plant(f0, tau, ws, kw["tau_lo"], kw["tau_hi"], dead, wp0)
    with np.errstate(invalid="ignore"):
        assert np.abs(f0).max() <= 1e4 and np.abs(wp).max() <= 2 and np.abs(ws).max() <= 2      # the premise of rule 2
    clean = np.where(np.isfinite(f), f, np.float32(0.0))
    c = Case()
    c.name, c.shape, c.regime, c.kw, c.dead = f"{shape} [{regime}]", shape, regime, kw, dead
    c.args, c.clean = (f, tau, wp, ws), (clean, tau, wp, ws)
    for a in c.args + (clean,):
        a.setflags(write=False)
    return c


# ------------------------------------------------------------------------------------------------- rule ---
def classify(x):
    """int8 class of every element: FINITE, C_NAN, C_PINF, C_NINF."""
    x = np.asarray(x)
    out = np.full(x.shape, FINITE, dtype=np.int8)
    out[np.isnan(x)] = C_NAN
    out[x == np.inf] = C_PINF
    out[x == -np.inf] = C_NINF
    return out


class Refs:
    """The float64 definition of one (case, out_of_bounds): ref the evaluation on the cleaned features (beam, B,
    computed), vol_class (K, N) the class of the evaluation on the planted ones (FINITE where nothing is computed)."""

    def counts(self):
        comp = self.ref.computed
        per_class = [int((comp & (self.vol_class == k)).sum()) for k in range(4)]
        any_comp = comp.any(axis=0)
        all_nan = int((any_comp & ~(comp & (self.vol_class != C_NAN)).any(axis=0)).sum())
        n_inf = (comp & (self.vol_class == C_PINF)).sum(axis=0)
        return dict(computed=int(comp.sum()), per_class=per_class, finite_share=per_class[FINITE] / max(1, int(comp.sum())),
                    all_nan_samples=all_nan, tied_inf_samples=int((n_inf > 1).sum()))

    def require(self):
        """The conditions of the module docstring: the inputs hold what the rule is about."""
        c = self.counts()
        assert c["finite_share"] >= MIN_FINITE_SHARE, (self.name, c)
        assert min(c["per_class"][1:]) >= MIN_PER_CLASS, (self.name, c)
        assert c["all_nan_samples"] >= MIN_ALL_NAN, (self.name, c)
        assert self.ref.K < TIED_FROM_K or c["tied_inf_samples"] >= MIN_TIED_INF, (self.name, c)
        return c


def strict_computed(tau, ws, N):
    """(K, N) bool: the beams strict bounds compute -- every term of a weighted station inside [0, N), and a weighted
    station at all (the build's conventions; f64_anchor.bp_f64 is the definition, the host test holds this against it)."""
    used = np.asarray(ws) != 0
    t64 = np.asarray(tau).astype(np.int64)
    lo = np.where(used[:, :, None], t64, np.iinfo(np.int64).max).min(axis=(1, 2))
    hi = np.where(used[:, :, None], t64, np.iinfo(np.int64).min).max(axis=(1, 2))
    t = np.arange(N)[None, :]
    has = used.any(axis=1)
    return has[:, None] & (t + np.where(has, lo, 0)[:, None] >= 0) & (t + np.where(has, hi, 0)[:, None] < N)


@functools.lru_cache(maxsize=8)
def _evaluations(shape, regime, seed):
    """The two float64 evaluations of a case under flexible bounds: on the cleaned and on the planted features.  A strict
    beam that is computed has every term inside the trace: it is the same sum."""
    c = case(shape, regime, seed)
    ref = fa.bp_f64(*c.clean, out_of_bounds="flexible")
    if regime == "int":
        # (the exact regime: cleaned integer features, every partial sum below 2^24 -- float32 equals float64)
        assert ref.mag.max() < fa.EXACT_LIMIT
        ref.B = np.zeros_like(ref.beam)
    with np.errstate(all="ignore"):
        bad = fa.bp_f64(*c.args, out_of_bounds="flexible")
    assert np.array_equal(bad.computed, ref.computed)
    return c, ref, bad.beam


def refs(shape, regime, oob, seed=0):
    c, flex, bad_beam = _evaluations(shape, regime, seed)
    r = Refs()
    r.name, r.case, r.oob = f"{c.name} {oob}", c, oob
    comp = flex.computed if oob == "flexible" else strict_computed(c.args[1], c.args[3], flex.N)
    r.ref = fa.BPRef()
    r.ref.times, r.ref.K, r.ref.N, r.ref.computed = flex.times, flex.K, flex.N, comp
    r.ref.beam, r.ref.B = np.where(comp, flex.beam, 0.0), np.where(comp, flex.B, 0.0)
    r.vol_class = classify(np.where(comp, bad_beam, 0.0))
    # a beam that is finite on the planted features read no bad sample: the cleaned evaluation is the same sum
    fin = comp & (r.vol_class == FINITE)
    assert np.array_equal(bad_beam[fin], flex.beam[fin])
    return r


def expected_max(ref, vol_class, first_computed):
    """Rule 3 per sample, from the definition: a dict of
    inf      (N,) bool: some computed beam is +Inf -- the maximum is (+Inf, inf_arg), exactly;
    inf_arg  (N,) the lowest source with a +Inf beam there;
    floor    (N,) bool: no computed beam is finite or +Inf (NaN and -Inf only, or nothing) -- (+0, id_offset) exactly,
             under either scan;
    finite   a BPRef restricted to the finite candidates of the samples without a +Inf: f64_anchor.bp_compare_max on it
             demands the floor where it holds no candidate, and elsewhere its three rules (and, under the default scan,
             the floor exactly where no candidate is > 0 beyond its bound)."""
    comp = ref.computed
    is_inf = comp & (vol_class == C_PINF)
    inf = is_inf.any(axis=0)
    cand = comp & (vol_class == FINITE) & ~inf[None, :]
    fin = fa.BPRef()
    fin.times, fin.K, fin.N = ref.times, ref.K, ref.N
    fin.computed, fin.beam, fin.B = cand, np.where(cand, ref.beam, 0.0), np.where(cand, ref.B, 0.0)
    return dict(inf=inf, inf_arg=is_inf.argmax(axis=0), floor=~inf & ~cand.any(axis=0), finite=fin,
                first_computed=first_computed)


# --------------------------------------------------------------------------------------------- checkers ---
def _at(mask):
    return tuple(int(x) for x in np.argwhere(mask)[0])


def check_none(got, r, oracle=None, what=""):
    """reduce="none": the class equal everywhere, +0 where not computed, finite beams inside B of the cleaned evaluation,
    and the oracle's output with NaNs at the same places."""
    got = np.asarray(got)
    what = what or r.name
    assert got.dtype == np.float32 and got.shape == r.vol_class.shape, (what, got.dtype, got.shape)
    cls = classify(got)
    bad = cls != r.vol_class
    assert not bad.any(), (f"{what}: class differs at (source, t) {_at(bad)}: got {got[_at(bad)]!r}, want "
                           f"{CLASS_NAMES[r.vol_class[_at(bad)]]} ({int(bad.sum())} beams)")
    bad = ~r.ref.computed & (got.view(np.uint32) != 0)
    assert not bad.any(), f"{what}: not +0 where nothing is computed, at {_at(bad)}: {got[_at(bad)]!r}"
    fin = r.ref.computed & (r.vol_class == FINITE)
    err = np.abs(np.where(fin, got, 0.0).astype(np.float64) - np.where(fin, r.ref.beam, 0.0))
    bad = fin & ~(err <= r.ref.B)
    assert not bad.any(), (f"{what}: finite beam outside its bound at {_at(bad)}: got {got[_at(bad)]!r}, cleaned f64 "
                           f"{r.ref.beam[_at(bad)]!r} +- {r.ref.B[_at(bad)]:.3e}")
    if oracle is not None:
        assert np.array_equal(got, oracle, equal_nan=True), \
            f"{what}: differs from the oracle at {_at(~((got == oracle) | (np.isnan(got) & np.isnan(oracle))))}"
    return float((err[fin] / np.maximum(r.ref.B[fin], 1e-300)).max(initial=0.0)) if (r.ref.B[fin] > 0).any() else 0.0


def check_max(m, a, r, first_computed=False, oracle=None, id_offset=0, what=""):
    """reduce="max": rule 3.  +Inf and floor samples exactly, finite maxima by f64_anchor.bp_compare_max on the cleaned
    reference restricted to the candidates, and the oracle's output bit for bit (its ids plus id_offset)."""
    m, a = np.asarray(m), np.asarray(a)
    what = what or r.name
    assert m.dtype == np.float32 and a.dtype == np.int32 and m.shape == a.shape == (r.ref.N,), (what, m.dtype, a.dtype, m.shape)
    assert not np.isnan(m).any(), f"{what}: a NaN max-beam at t {_at(np.isnan(m))}"
    exp = expected_max(r.ref, r.vol_class, first_computed)
    src = a.astype(np.int64) - id_offset
    bad = exp["inf"] & ~((m == np.inf) & (src == exp["inf_arg"]))
    assert not bad.any(), (f"{what}: a +Inf beam is the maximum, lowest source first: at t {_at(bad)} got "
                           f"({m[_at(bad)]!r}, {src[_at(bad)]}), want (inf, {exp['inf_arg'][_at(bad)]})")
    bad = exp["floor"] & ~((m.view(np.uint32) == 0) & (src == 0))
    assert not bad.any(), f"{what}: floor (+0, id_offset) at t {_at(bad)}: got ({m[_at(bad)]!r}, {a[_at(bad)]})"
    bad = ~exp["inf"] & ~np.isfinite(m)
    assert not bad.any(), f"{what}: {m[_at(bad)]!r} at t {_at(bad)} where no computed beam is +Inf"
    keep = ~exp["inf"]
    rep = fa.bp_compare_max(np.where(keep, m, np.float32(0.0)), np.where(keep, src, 0).astype(np.int32), exp["finite"],
                            first_computed, what + " finite maxima")
    assert rep.n_bad == 0, f"{what}: {rep.n_bad} of {rep.n} finite maxima outside the rules; {rep.detail}"
    if oracle is not None:
        wm, wa = oracle
        assert np.array_equal(m, wm), f"{what}: max-beam differs from the oracle at t {_at(m != wm)}"
        assert np.array_equal(src, wa), f"{what}: arg-max differs from the oracle at t {_at(src != wa)}"
    return rep.worst


# ------------------------------------------------------------------- the scan, in NumPy, with planted defects ---
DEFECTS_MAX = ("nan_wins", "nan_first_sticks", "inf_tie_highest_id", "neg_inf_beats_floor", "first_computed_keeps_neg_inf")
DEFECTS_BEAM = ("zero_weight_station_multiplies", "zero_phase_weight_skipped", "flexible_clamps_to_edge",
                "strict_uncomputed_leaks")
DEFECTS = DEFECTS_MAX + DEFECTS_BEAM


def scan_max(vol, computed, first_computed=False, defect=None):
    """Rule 3 from a float32 (K, N) volume and its computed mask: (max-beam, arg-max) -- or, with `defect` one of
    DEFECTS_MAX, what a scan with that defect returns; then a third value tells whether any sample changed."""
    vol = np.asarray(vol)
    K, N = vol.shape
    j = np.arange(N)
    is_nan = computed & np.isnan(vol)
    cand = computed & ~is_nan
    masked = np.where(cand, vol, -np.inf)
    best, arg = masked.max(axis=0), masked.argmax(axis=0)
    keep = (cand.any(axis=0) & (best > -np.inf)) if first_computed else best > 0
    m, a = np.where(keep, best, 0.0).astype(np.float32), np.where(keep, arg, 0).astype(np.int32)
    if defect is None:
        return m, a
    assert defect in DEFECTS_MAX
    if defect == "nan_wins":                          # `!(acc <= best)`: a NaN beam replaces the maximum
        hit = is_nan.any(axis=0)
        m[hit], a[hit] = NAN, is_nan.argmax(axis=0)[hit]
    elif defect == "nan_first_sticks":                # the scan starts from the first computed beam: a NaN there stays
        first = computed.argmax(axis=0)
        hit = computed.any(axis=0) & np.isnan(vol[first, j])
        m[hit], a[hit] = NAN, first[hit]
    elif defect == "inf_tie_highest_id":
        is_inf = cand & (vol == np.inf)
        hit = is_inf.sum(axis=0) > 1
        a[hit] = (K - 1 - is_inf[::-1].argmax(axis=0))[hit]
    elif defect == "neg_inf_beats_floor":             # the floor compared with >= -Inf, or left out
        is_ninf = cand & (vol == -np.inf)
        hit = ~keep & is_ninf.any(axis=0) & (not first_computed)
        m[hit], a[hit] = NINF, is_ninf.argmax(axis=0)[hit]
    else:                                             # first_computed: a maximum of -Inf handed out
        hit = cand.any(axis=0) & (best == -np.inf) & bool(first_computed)
        m[hit], a[hit] = NINF, arg[hit]
    return m, a, bool(hit.any())


def _bad_prestack(f):
    """(S, 1, N) bool: U[s, p, t] is non-finite (rule 1: for every phase as soon as one component is)."""
    return ~np.isfinite(f).all(axis=1)[:, None, :]


def defective(name, r, oracle):
    """The (K, N) float32 volume of the definition with one of DEFECTS_BEAM planted into the case of `r` (a Refs), or None
    where the case does not name it (`oracle`: the module oracle.oracle).  The maximum of a defective volume is scan_max
    of it over the same computed mask -- every beam computed under "strict_uncomputed_leaks"."""
    assert name in DEFECTS_BEAM
    f, tau, wp, ws = r.case.args
    oob, computed = r.oob, r.ref.computed
    S, C, N = f.shape
    K, _, P = tau.shape
    vol = oracle.beamform(f, tau, wp, ws, oob, "none")
    t = np.arange(N)[None, :]
    if name == "zero_phase_weight_skipped":           # `if (alpha == 0) continue;` in the prestack
        f2 = f.copy()
        dead_c = (wp == 0).all(axis=2)
        f2[dead_c] = np.where(np.isfinite(f2[dead_c]), f2[dead_c], np.float32(0.0))
        out = oracle.beamform(f2, tau, wp, ws, oob, "none")
    elif name == "strict_uncomputed_leaks":           # the select behind the accumulation left out
        if oob != "strict":
            return None
        has = (ws != 0).any(axis=1)
        out = np.where(has[:, None], oracle.beamform(f, tau, wp, ws, "flexible", "none"), np.float32(0.0))
    else:
        badU = _bad_prestack(f)
        hit = np.zeros((K, N), dtype=bool)
        for s in range(S):
            for p in range(P):
                x = t + tau[:, s, p].astype(np.int64)[:, None]
                inb = (x >= 0) & (x < N)
                xc = np.clip(x, 0, N - 1)
                if name == "zero_weight_station_multiplies":      # fmaf(0, U, b) instead of the skip
                    hit |= (ws[:, s] == 0)[:, None] & inb & badU[s, 0][xc]
                elif oob == "flexible":                           # a dropped term reads sample 0 or N - 1
                    hit |= (ws[:, s] != 0)[:, None] & ~inb & badU[s, 0][xc]
        hit &= computed
        out = np.where(hit, NAN, vol)
    same = (out == vol) | (np.isnan(out) & np.isnan(vol))
    return None if same.all() else out.astype(np.float32)


# -------------------------------------------------------------------------------------------- relocation ---
def focus_of_volume(vol, computed=None):
    """Rule 4 stated on the volume: the first maximum in source-major order over the entries that are not NaN (every
    entry counts, +0 of a beam that is not computed included): (src_idx, time_idx); (0, 0) for a volume of NaN."""
    vol = np.asarray(vol)
    masked = np.where(np.isnan(vol), -np.inf, vol)
    k, t = np.unravel_index(masked.argmax(), vol.shape)
    return int(k), int(t)


def relocation_events(regime, seed=0):
    """(E = 4, S, C, N) features of the relocation case and its tables: event 0 planted, event 1 clean, event 2 all NaN,
    event 3 clean but for one +Inf sample."""
    c0 = case("relocation", regime, seed)
    f0, tau, wp, ws = c0.args
    kw = SHAPES["relocation"][0]
    others = [fa.bp_case(regime, seed=40 + e, **kw)[0] for e in (1, 2, 3)]
    others[1][:] = NAN
    s = int(np.flatnonzero(ws[7] != 0)[0])
    others[2][s, int(np.argmax(wp[s, :, 0] != 0)), kw["N"] // 2] = PINF
    f = np.stack([f0] + others)
    f.setflags(write=False)
    return f, tau, wp, ws
