"""Cases and the one checker of the template builder (csrc/templates.hip, workflow.templates_from_events,
postprocess.templates_from_events_host), shared by tests/test_templates_host.py (CPU) and
tests/test_gpu_templates.py (GPU).

A case is a day (S, C, N), E origins, (E, S, C) window moveouts, a window length L, a `normalize` mode and an optional
noise window.  The channels of a day are of eight kinds, rotated from case to case (KINDS), and the windows of a case
go through eleven placements (PLACEMENTS): every (event, channel) gets the next one.  CASES crosses the lengths at
which NumPy's pairwise sum changes shape -- 1, 7 | 8, 9 (running sum | eight accumulators), 127, 128 | 129, 136 (one
leaf | two), 257 (an uneven tree), 1000, 4096, 8192 (the ceiling) -- with S * C in {1, 5, 60} and E in {1, 3, 300},
each `normalize` mode, with and without the SNR.

The checker (`check`) compares bit for bit through view(uint32); NaNs must sit at the same positions, their payloads
are not compared."""
import numpy as np

LENGTHS = (1, 7, 8, 9, 127, 128, 129, 136, 257, 1000, 4096, 8192)
KINDS = ("normal", "zero", "constant", "nan", "inf", "negative_zero", "tiny20", "tiny30")
PLACEMENTS = ("at_start", "at_end", "cut_by_start", "cut_by_end", "before_day", "past_day", "inside", "one_in",
              "one_left", "inside", "touching_end_from_outside")
FLOAT_KEYS = ("templates", "norm", "snr")
BOOL_KEYS = ("available", "complete")


def channel(rng, kind, n):
    """One channel of a day, of one of KINDS."""
    x = rng.standard_normal(n).astype(np.float32)
    if kind == "zero":
        x[:] = 0.0
    elif kind == "constant":
        x[:] = np.float32(3.3)
    elif kind == "nan":                         # sparse: some windows hold one, some none
        x[rng.integers(0, n, max(1, n // 3000))] = np.nan
        x[: n // 2] = 0.0                       # and windows that are all zero but for a NaN
        x[n // 16] = np.nan
    elif kind == "inf":
        p = rng.integers(0, n, max(2, n // 3000))
        x[p[::2]] = np.inf
        x[p[1::2]] = -np.inf
    elif kind == "negative_zero":
        x[rng.random(n) < 0.3] = -0.0
        x[: n // 2] = -0.0                      # whole windows of -0.0: not available, norm 1, templates -0.0
    elif kind == "tiny20":                      # squares are subnormal
        x *= np.float32(1e-20)
    elif kind == "tiny30":                      # squares underflow: std 0, norm 1
        x *= np.float32(1e-30)
    return x


def window_start(rng, placement, n, L):
    """i0 of a window of one of PLACEMENTS in a day of n samples."""
    return {"at_start": 0, "at_end": n - L, "cut_by_start": -((L + 1) // 2), "cut_by_end": n - L // 2,
            "before_day": -L - 3, "past_day": n + 2, "one_in": -L + 1, "one_left": n - 1,
            "touching_end_from_outside": n}.get(placement, int(rng.integers(0, max(1, n - L + 1))))


def make_case(seed, S, C, E, L, normalize="rms", noise=None, n=None, rotate=0, placements=PLACEMENTS):
    """One case as a dict: data (S, C, N) float32, origin (E,) int64, moveouts (E, S, C) int32 (most of them negative
    or large: the placement decides, not the origin), L, normalize, noise_offset / noise_samples (None: no SNR)."""
    rng = np.random.default_rng(seed)
    n_noise = 0 if noise is None else noise[1]
    n = max(3 * L, 2 * n_noise, 64) + 37 if n is None else n
    kinds = [KINDS[(ch + rotate) % len(KINDS)] for ch in range(S * C)]
    data = np.stack([channel(rng, k, n) for k in kinds]).reshape(S, C, n)
    origin = rng.integers(0, n, E).astype(np.int64)
    if noise is not None and E:
        origin[0] = noise[0] // 2               # the first event's noise window is cut by the start of the day
        origin[-1] = n + noise[0] + 1           # the last one's lies wholly past the day (noise std 0)
    mv = np.zeros((E, S, C), dtype=np.int32)
    place = np.empty((E, S, C), dtype=object)
    k = int(rng.integers(0, len(placements)))
    for e in range(E):
        for s in range(S):
            for c in range(C):
                place[e, s, c] = placements[k % len(placements)]
                mv[e, s, c] = window_start(rng, place[e, s, c], n, L) - origin[e]
                k += 1
    return {"data": data, "origin": origin, "moveouts": mv, "L": L, "normalize": normalize,
            "noise_offset": None if noise is None else noise[0], "noise_samples": None if noise is None else noise[1],
            "kinds": np.array(kinds).reshape(S, C), "placement": place}


def _cases():
    """(label, make_case arguments): every length with S * C = 5 and E = 3, the modes and noise windows taking turns;
    then the channel and event counts at lengths of one and two leaves."""
    out = []
    modes = ("rms", "max", None)
    for i, L in enumerate(LENGTHS):
        n_noise = LENGTHS[(2 * i + 5) % len(LENGTHS)]               # every length is a noise length too
        # none | wholly before the origin | reaching past the origin, into the signal windows
        noise = (None, (n_noise + 11, n_noise), (n_noise // 2, n_noise))[i % 3]
        out.append((f"L={L}", dict(seed=500 + i, S=1, C=5, E=3, L=L, normalize=modes[i % 3], noise=noise, rotate=i)))
    for j, (S, C, E, L) in enumerate([(1, 1, 1, 136), (1, 1, 3, 9), (1, 1, 300, 129), (20, 3, 1, 257), (20, 3, 3, 128),
                                      (20, 3, 300, 136), (1, 5, 300, 8), (1, 5, 1, 1000)]):
        out.append((f"S*C={S * C} E={E} L={L}", dict(seed=600 + j, S=S, C=C, E=E, L=L, normalize=modes[(j + 1) % 3],
                                                     noise=(40, 100) if j % 2 else None, rotate=j)))
    # every mode with and without the SNR on one shape, and rms at the ceiling of both lengths
    for j, mode in enumerate(modes):
        for noise in (None, (300, 257)):
            out.append((f"mode={mode} noise={noise}", dict(seed=700 + j, S=2, C=4, E=3, L=200, normalize=mode,
                                                           noise=noise, rotate=j)))
    out.append(("ceilings", dict(seed=720, S=1, C=5, E=3, L=8192, normalize="rms", noise=(8192, 8192), rotate=3)))
    return out


CASES = _cases()


def host_answer(case):
    from seismic_bpmf_amd import postprocess as pp
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        return pp.templates_from_events_host(case["data"], case["origin"], case["moveouts"], case["L"],
                                             case["normalize"], case["noise_offset"], case["noise_samples"])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def check(got, want, label=""):
    """AssertionError unless `got` (a dict with templates, norm, available, complete, snr as NumPy arrays) equals the
    definition's answer `want` bit for bit, NaNs at the same positions."""
    for key in BOOL_KEYS:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.dtype == np.bool_ and g.shape == w.shape, f"{label}: {key} is {g.dtype} {g.shape}, want bool {w.shape}"
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError(f"{label}: {key} differs at {len(bad)} of {w.size} channels, first (e, s, c) = "
                                 f"{tuple(bad[0])}: got {g[tuple(bad[0])]}")
    assert (got["snr"] is None) == (want["snr"] is None), f"{label}: snr given {got['snr'] is not None}"
    for key in FLOAT_KEYS:
        if want[key] is None:
            continue
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.dtype == np.float32 and g.shape == w.shape, f"{label}: {key} is {g.dtype} {g.shape}, want {w.shape}"
        if not same_bits(g, w):
            bad = np.argwhere(~((g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))))
            i = tuple(bad[0])
            raise AssertionError(f"{label}: {key} differs at {len(bad)} of {w.size} elements, first at {i}: got "
                                 f"{g[i]!r} ({g.view(np.uint32)[i]:#010x}), want {w[i]!r} ({w.view(np.uint32)[i]:#010x})")


def classes_met(case, want):
    """The names of the special situations the comparison of this case went through (a set)."""
    met = set()
    kinds, place = case["kinds"], case["placement"]
    for e, s, c in np.ndindex(*place.shape):
        met.add("placement:" + place[e, s, c])
        met.add("kind:" + kinds[s, c])
        if case["moveouts"][e, s, c] < 0:
            met.add("negative_moveout")
        inside = place[e, s, c] in ("at_start", "at_end", "inside")
        if inside and kinds[s, c] == "tiny30" and case["L"] > 1 and case["normalize"] == "rms" \
                and want["norm"][e, s, c] == 1.0 and want["available"][e, s, c]:
            met.add("underflow_norm_1")
        if inside and kinds[s, c] == "tiny20" and case["L"] > 1 and case["normalize"] == "rms" \
                and 0.0 < want["norm"][e, s, c] < 1e-19:
            met.add("subnormal_squares")
        if np.isnan(want["norm"][e, s, c]):
            met.add("nan_norm")
        if want["available"][e, s, c] and np.isnan(want["templates"][e, s, c]).all():
            met.add("nan_channel_available")
        if not want["available"][e, s, c] and np.signbit(want["templates"][e, s, c]).any():
            met.add("negative_zero_window")
        if want["snr"] is not None:
            met.add("snr")
            j0 = int(case["origin"][e]) - case["noise_offset"]
            if j0 < 0 < j0 + case["noise_samples"]:
                met.add("noise_cut_by_start")
            i0 = int(case["origin"][e]) + int(case["moveouts"][e, s, c])
            if max(i0, j0) < min(i0 + case["L"], j0 + case["noise_samples"]):
                met.add("noise_overlaps_signal")
            if kinds[s, c] in ("zero", "tiny30") or j0 >= case["data"].shape[-1]:
                met.add("noise_std_0")
    met.add(f"normalize:{case['normalize']}")
    return met


ALL_CLASSES = ({"placement:" + p for p in PLACEMENTS} | {"kind:" + k for k in KINDS} |
               {"negative_moveout", "underflow_norm_1", "subnormal_squares", "nan_norm", "nan_channel_available",
                "negative_zero_window", "snr", "noise_cut_by_start", "noise_overlaps_signal", "noise_std_0",
                "normalize:rms", "normalize:max", "normalize:None"})
