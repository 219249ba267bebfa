"""CPU: which kernel a matched-filter launch takes (bpmf_mf_launch_info = mf_choose of csrc/mf.hip).

Every kernel family gives the same bits, so a slip in the choice would show only as lost speed on a GPU.  Here
the rules are restated in Python, independently of the C++ (written from the launch code as it stood before the
choice was gathered into one function), and compared with the library field by field on every boundary of the
choice.  The info call allocates nothing and needs no device: large sizes are free."""
import pytest

from seismic_bpmf_amd import _lib

FORCE_DIRECT = 2            # BPMF_MF_FORCE_DIRECT
DEFAULTS = {"mf.wave_kernel": 1, "mf.max_mfma_step": 64, "mf.tiles_per_wave": 0, "mf.fused_prologue": 1,
            "mf.channel_split": 2048, "mf.split16": 0, "mf.compat_sqrt_norm": 0}


def ceil_div(a, b):
    return (a + b - 1) // b


def expected(step, L, N, T, S, C, network_sum=True, flags=0, **opts):
    o = dict(DEFAULTS, **{k.replace("__", "."): v for k, v in opts.items()})
    n_ch = S * C
    n_corr = (N - L) // step + 1
    n_offsets = (n_corr - 1) * step + 1             # the MFMA kernels evaluate every data offset
    n_lag_blocks = ceil_div(n_offsets, 4096)
    kpad = (L + 30) // 16 * 16
    window, band = 4096 - 16 + kpad, kpad + 16
    need_r, need_t = ceil_div(window, 256), ceil_div(band, 256)
    v = dict(family="direct", maxr=0, maxt=0, ntile=0, fused=False, csplit=False,
             sqrt_norm=bool(o["mf.compat_sqrt_norm"]), step1=step == 1, prologue=True, lags_per_wg=256, lds_bytes=0,
             grid=ceil_div(n_corr, 256) * T, refusal=None)
    mfma = (step <= o["mf.max_mfma_step"] and not flags & FORCE_DIRECT and need_r <= 24 and need_t <= 9 and
            T * (n_lag_blocks + 8) < 0x7fffffff and N < 2 ** 30 - 8192)
    if not mfma:
        if T > 65535:
            v["refusal"] = "more than 65535 templates on the generic kernel"
        return v
    grid8 = lambda n_blocks: 8 * ceil_div(T * n_blocks, 8)
    sp_blocks = ceil_div(n_offsets, 8192)
    sp_usable = L <= 4096 and N < 2 ** 30 - 8192
    if o["mf.split16"] and sp_usable and not (o["mf.split16"] == 1 and T * sp_blocks < 128):
        v.update(family="split16", lags_per_wg=8192, grid=grid8(sp_blocks))
        return v
    if not (o["mf.wave_kernel"] and kpad <= 272):
        small = need_r <= 20 and need_t <= 5
        buf = band + window + (window >> 4) + 1
        v.update(family="workgroup", maxr=20 if small else 24, maxt=5 if small else 9, lags_per_wg=4096,
                 lds_bytes=(2 * buf + 64) * 4, grid=grid8(n_lag_blocks))
        return v
    waves4 = 4 * T * n_lag_blocks
    ntile = 4 if waves4 >= 8192 else 2 if waves4 >= 1024 else 1
    if o["mf.tiles_per_wave"] in (1, 2, 4):
        ntile = o["mf.tiles_per_wave"]
    fused = ntile < 4 and n_ch <= 256 and bool(o["mf.fused_prologue"])
    csplit = (ntile == 1 and fused and bool(network_sum) and step == 1 and n_ch <= 32 and
              o["mf.channel_split"] > 0 and 4 * waves4 <= o["mf.channel_split"])
    lags_wg = 256 if csplit else 1024 * ntile
    n_blocks = ceil_div(n_offsets, lags_wg)
    maxr = {4: 20, 2: 12, 1: 8}[ntile]
    wbuf = 64 * maxr if ntile < 4 else 256 * ntile - 16 + kpad
    lds = (4 * (band + (wbuf + 2 * (wbuf >> 4) + 2 + 63) // 64 * 64 + 64) * 4 + 256 +
           (64 + (n_ch + 12) * 16 if fused else 0) + (n_ch * 256 * 4 if csplit else 0))
    v.update(family="wave", maxr=maxr, maxt=5, ntile=ntile, fused=fused, csplit=csplit, prologue=not fused,
             lags_per_wg=lags_wg, lds_bytes=lds, grid=grid8(n_blocks),
             refusal="grid too large" if T * (n_blocks + 8) >= 0x7fffffff else None)
    return v


def case(L=64, n_offsets=4096, step=1, T=3, S=5, C=3, N=None, **kw):
    """A launch of `n_offsets` data offsets at step 1 (one lag block of the MFMA kernels = 4096 of them)."""
    return dict(step=step, L=L, N=N if N is not None else n_offsets + L - 1, T=T, S=S, C=C, **kw)


CASES = []
# template length: wave kernel to 257, workgroup (20, 5) to 1025, (24, 9) to 2049, then the generic kernel
CASES += [case(L=L, N=30000) for L in (1, 257, 258, 1025, 1026, 2049, 2050)]
# mf.wave_kernel = 0: the workgroup kernel (20, 5) at the wave kernel's lengths
CASES += [case(L=L, N=30000, mf__wave_kernel=0) for L in (1, 257, 258)]
# step: the MFMA kernels to mf.max_mfma_step
CASES += [case(step=s, N=30000) for s in (1, 3, 64, 65)]
CASES += [case(step=s, N=30000, network_sum=False) for s in (1, 3)]
CASES += [case(N=30000, flags=FORCE_DIRECT), case(N=30000, mf__max_mfma_step=0), case(N=30000, step=3, mf__max_mfma_step=2)]
# tiles per wave by the waves of the whole problem: 1020 / 1024 and 8188 / 8192 at one lag block, 1024 over two
CASES += [case(T=T) for T in (255, 256, 2047, 2048)]
CASES += [case(T=128, n_offsets=4097), case(T=127, n_offsets=4097), case(T=1024, n_offsets=8192), case(T=1024, n_offsets=8193)]
CASES += [case(T=T, mf__tiles_per_wave=f) for T in (3, 300, 3000) for f in (0, 1, 2, 3, 4)]
# fused prologue: fewer than 4 tiles, at most 256 channels, the option
CASES += [case(T=T, S=S, C=1, mf__fused_prologue=f) for T in (3, 300, 3000) for S in (256, 257) for f in (0, 1)]
# channel split: one tile, fused, network sum, step 1, <= 32 channels, 16 T <= mf.channel_split at one lag block
CASES += [case(T=T, S=S, C=1) for T in (128, 129) for S in (32, 33)]
CASES += [case(T=128, S=32, C=1, network_sum=False), case(T=128, S=32, C=1, step=3, N=4096 + 63),
          case(T=128, S=32, C=1, mf__fused_prologue=0), case(T=128, S=32, C=1, mf__tiles_per_wave=2),
          case(T=128, S=32, C=1, mf__channel_split=0), case(T=128, S=32, C=1, mf__channel_split=2047),
          case(T=200, S=32, C=1, mf__channel_split=3200), case(T=201, S=32, C=1, mf__channel_split=3200),
          case(T=64, S=32, C=1, n_offsets=4097), case(T=65, S=32, C=1, n_offsets=4097)]
# mf.split16: 1 from 128 (template, 8192-lag block) pairs on, 2 always; lengths / traces its arithmetic cannot take
CASES += [case(T=T, n_offsets=8192, mf__split16=m) for T in (127, 128) for m in (0, 1, 2)]
CASES += [case(T=T, n_offsets=8193, mf__split16=1) for T in (63, 64)]
CASES += [case(L=2049, N=30000, mf__split16=2), case(L=2050, N=30000, mf__split16=2), case(L=4097, N=30000, mf__split16=2),
          case(N=2 ** 30 - 8193, mf__split16=2), case(N=2 ** 30 - 8192, mf__split16=2),
          case(N=30000, step=65, mf__split16=2), case(N=30000, flags=FORCE_DIRECT, mf__split16=2)]
# mf.compat_sqrt_norm: a template argument of every family
CASES += [case(L=L, N=30000, mf__compat_sqrt_norm=q) for L in (64, 300, 2050) for q in (0, 1)]
CASES += [case(N=30000, mf__compat_sqrt_norm=1, mf__split16=2)]
# traces of 2^30 - 8192 samples or more: the generic kernel
CASES += [case(N=2 ** 30 - 8193), case(N=2 ** 30 - 8192), case(L=300, N=2 ** 30 - 8193), case(L=300, N=2 ** 30 - 8192)]
# T * (lag blocks + 8) against 2^31 - 1: at one lag block 9 T, at two 10 T
CASES += [case(T=238609294, S=1, C=1), case(T=238609295, S=1, C=1),
          case(T=214748364, S=1, C=1, n_offsets=4097), case(T=214748365, S=1, C=1, n_offsets=4097),
          case(L=300, T=238609294, S=1, C=1), case(L=300, T=238609295, S=1, C=1)]
# ... and of the wave kernel's own blocks: 1024 lags each at one tile per wave, 12 T
CASES += [case(T=178956970, S=1, C=1, mf__tiles_per_wave=1), case(T=178956971, S=1, C=1, mf__tiles_per_wave=1)]
# the generic kernel: at most 65535 templates
CASES += [case(T=T, N=30000, flags=FORCE_DIRECT) for T in (65535, 65536)]
CASES += [case(T=T, L=2050, N=30000, S=1, C=1) for T in (65535, 65536)]


def case_id(c):
    return "-".join(f"{k.replace('mf__', '')}={v}" for k, v in c.items())


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_choice_equals_its_restatement(hip_opts, c):
    args = {{"S": "n_stations", "C": "n_components"}.get(k, k): v for k, v in c.items() if "__" not in k}
    for k, v in c.items():
        if "__" in k:
            hip_opts(k.replace("__", "."), v)
    got = _lib.mf_launch_info(**args)
    want = expected(**c)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], (name, got, want)


def test_cases_reach_every_answer():
    """The cases above are on both sides of every rule: each family, each compiled register variant, each tile
    count with and without the fused prologue, the channel split, both refusals."""
    seen = [expected(**c) for c in CASES]
    assert {v["family"] for v in seen} == set(_lib.MF_FAMILIES)
    assert {(v["maxr"], v["maxt"]) for v in seen if v["family"] == "workgroup"} == {(20, 5), (24, 9)}
    assert {(v["ntile"], v["fused"], v["csplit"]) for v in seen if v["family"] == "wave"} == \
        {(4, False, False), (2, False, False), (2, True, False), (1, False, False), (1, True, False), (1, True, True)}
    assert {v["refusal"] for v in seen} == set(_lib.MF_REFUSALS)
    assert {v["sqrt_norm"] for v in seen} == {False, True} and {v["step1"] for v in seen} == {False, True}


def test_restated_defaults_are_the_library_s():
    for name, value in DEFAULTS.items():
        assert _lib.get_option(name) == (value, value), name


def test_info_checks_sizes_like_the_launch():
    with pytest.raises(_lib.BpmfHipError, match="zero-sized"):
        _lib.mf_launch_info(1, 64, 30000, 0, 5, 3)
    with pytest.raises(_lib.BpmfHipError, match="shorter than the templates"):
        _lib.mf_launch_info(1, 64, 63, 3, 5, 3)
