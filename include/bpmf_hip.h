/*
 * bpmf_hip.h -- C ABI of libbpmf_hip.so, the MI355X (gfx950) implementation of the two
 * data-parallel hot paths of the Seismic_BPMF workflow.
 *
 * Conventions (mirroring the reference's own ctypes layer, BPMF/clib.py:14-84 and
 * BPMF/libc.h:1-11): plain C symbols, C-contiguous float32 / int32 arrays, sizes as
 * size_t, the caller allocates every output.  Unlike the reference (all functions
 * return void and report problems with printf) every entry point returns an int status:
 * 0 = ok, -1 = bad argument, -2 = HIP runtime error; bpmf_last_error() gives the text.
 *
 * Two flavours per path:
 *   *_run      host pointers in / host pointers out (what a ctypes wrapper of the
 *              reference's third-party back-ends binds; does H2D, kernels, D2H);
 *   *_run_dev  device pointers, asynchronous on the given HIP stream, caller-provided
 *              workspace (what the resident / multi-GPU / benchmark path uses).
 *
 * Memory contract of every device-pointer entry point (tests/test_gpu_guard_bands.py runs each of them between
 * guard bands, on a workspace of exactly the size its bpmf_*_workspace_bytes names):
 *   - it writes no byte outside its outputs and [d_workspace, d_workspace + workspace_bytes); a call that is
 *     refused (-1) writes nothing at all, the fill of option debug.poison_output included;
 *   - it reads nothing of the workspace that the same call -- or the preparation its flags name
 *     (BPMF_MF_DATA_PREPARED) -- has not written: the results do not depend on what the workspace held before, nor
 *     on which of the accepted sizes it has;
 *   - a bpmf_*_workspace_bytes function returns 0 for sizes that its call refuses (a zero dimension, a series shorter
 *     than its window, more rows than one call takes) and never less for more rows;
 *   - it expects every buffer aligned as the device allocator aligns it (256 bytes); finer alignments are the
 *     caller's risk unless an entry point says otherwise.
 *
 * The hot-path arithmetic itself is NOT in the reference tree: BPMF calls the external
 * packages fast_matched_filter and beampower (pyproject.toml:28-29).  Each entry point
 * cites the reference call site it serves.
 */
#ifndef BPMF_HIP_H
#define BPMF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *bpmf_stream_t; /* a hipStream_t; NULL = the default stream */

/* ---------------------------------------------------------------- diagnostics --- */

/* Text of the last error raised on the calling thread ("" if none). */
const char *bpmf_last_error(void);

/* Number of visible HIP devices (<0 on runtime error).
 * Replaces the device query of BPMF/GPU.cu:8-24 (caract_GPU). */
int bpmf_device_count(void);

/* Name, memory and compute-unit count of one device.  BPMF/GPU.cu:14-22. */
int bpmf_device_info(int device, char *name, size_t name_len, size_t *total_mem_bytes,
                     int *compute_units);

/* Optional timing of the dominant kernel of each path with HIP events recorded on the
 * caller's stream (used by bench.py for the roofline figure; off by default).
 * Each launch of the kernel logs its own event pair; read them after synchronising.
 * (The reference only has wall-clock prints: BPMF/similarity_search.py:789-806.) */
#define BPMF_KERNEL_MF_MAIN 0
#define BPMF_KERNEL_BP_BEAM 1
#define BPMF_KERNEL_COUNT 2
void bpmf_profile_enable(int enable); /* enabling clears the log; disabling keeps it */
int bpmf_profile_count(int which_kernel); /* launches logged since enable */
int bpmf_profile_get_ms(int which_kernel, int launch_index, float *milliseconds);
/* The device that launch ran on (-1: no such launch).  Launches made by several host threads (the
 * *_multi entry points: one thread per GPU) are logged per thread and per device: a start edge and
 * a stop edge pair up only on the thread that recorded both. */
int bpmf_profile_get_device(int which_kernel, int launch_index);

/* The host-pointer entry points (bpmf_mf_run, bpmf_bp_run, their *_multi forms,
 * bpmf_find_similar_sources) keep, per device and process: two private streams, a side stream, four
 * events, two pinned staging pieces and the device working set of the largest recent call -- created
 * once, reused by every call, never destroyed while the library is loaded; calls on one device take
 * turns (the reference's counterpart: the third-party back-ends allocate and free per call,
 * BPMF/similarity_search.py:526-533, BPMF/template_search.py:549-558).  bpmf_release_device_memory
 * gives the working set and the pinned pieces back (device < 0: every device; waits for a running
 * call); bpmf_device_memory_held reports what is held right now; option host.cache_limit_mb (0 = no limit) gives a
 * working set above the limit back at the end of the call that needed it.  The *_dev entry points hold nothing. */
int bpmf_release_device_memory(int device);
int bpmf_device_memory_held(int device, size_t *device_bytes, size_t *pinned_bytes);
/* Where the time of the calling thread's LAST host-pointer call went (bpmf_bp_run / bpmf_mf_run, or the first
 * device's block of a *_run_multi call made from this thread), milliseconds on the host clock:
 *   out[0] the whole call; out[1] from entry to the first kernel being enqueued (plan lookup, working set, the
 *   first piece of the day through the pinned buffers); out[2] host threads copying the day into the pinned
 *   pieces (summed over the pieces; overlaps the kernels of earlier pieces); out[3] waiting for the device after
 *   the last launch was enqueued (kernels still running + the results' way back); out[4] pieces the day arrived
 *   in; out[5] host threads that filled them; out[6] waiting for a pinned piece to be free again (its previous
 *   copy still in flight); out[7] inside the runtime's asynchronous-copy calls of the pieces;
 *   out[8] finding (or building) the backprojection plan; out[9] reserving the device working set and the pinned pieces;
 *   out[10] stragglers: blocks of a pinned piece's fill that the calling thread copied itself while a copy-pool thread
 *   still held them (that thread writes the same bytes later; nothing else writes into the piece before it is done).
 *   Returns the number of values written (<= n).  The reference has no
 *   counterpart (its back-ends' calls are opaque, BPMF/template_search.py:549-558); bench.py reports these beside
 *   the end-to-end times. */
int bpmf_host_call_stats(double *out, int n);

/* Execution options.  The library reads NOTHING from the environment.  An option selects among
 * code paths and sizes that produce identical results (kernel family, LDS budget, batch sizes of
 * the host-pointer calls, group ranges per tile): the GPU tests use them to drive every kernel
 * family through the same parity cases, tools/ to measure alternatives.  Process-wide, thread
 * safe; plans already built keep the variant they were built with.  Names:
 *   bp.lds_kb bp.max_group bp.tpt (1 or 2) bp.reorder bp.dual bp.fast
 *   bp.fast_uniform bp.fast_tile bp.halves bp.direct bp.split bp.slot_prio bp.verbose
 *   mf.wave_kernel mf.tiles_per_wave mf.boundary_prio mf.fused_prologue mf.channel_split mf.max_mfma_step mf.host_batch_kb mf.host_piece_kb mf.verbose
 *   stats.bucketed_median (MAD threshold, window medians: 2 one pass each, 1 two passes, 0 radix select only)
 *   stats.row_grid_min_n (row median / MAD: rows at least this long are read twice by the whole chip; -1 never)
 *   stats.kurt_full_chunks (row kurtosis: full 8192-sample chunks summed by one workgroup each through LDS)
 *   mf.host_piece_lags bp.host_piece_samples (host-pointer calls: the day arrives in pieces while the first kernels run; 0 = off)
 *   debug.poison_output (tests: outputs pre-filled with 0xFF bytes, so that a sample no kernel writes shows)
 *   debug.virtual_devices (tests: k > 0 makes every `device` argument a LOGICAL device 0 .. k-1, logical d on
 *     physical GPU d % visible, each with its own streams / working set / call mutex and, in the *_run_multi
 *     entry points, its own host thread: the multi-device branches run on a box with one GPU;
 *     bpmf_device_count then reports k)
 *   multi.peer_fanout (*_run_multi on several devices: 1 = the first device uploads the day of data from the
 *     host ONCE and the others copy it device -> device, hipMemcpyPeerAsync over xGMI; 0 = every device
 *     uploads from the host itself, which is what the upstream back-ends do)
 *     a device-to-device copy the platform refuses falls back to host uploads for that device, status 0, with a
 *     "note: ..." in bpmf_last_error; debug.fail_peer_copy (tests) makes every copy be refused
 *   debug.copy_stall_ms (tests, 0 .. 2000: k > 0 = in every multi-block fill of a pinned piece by the copy pool, the
 *     pool thread that draws the first block sleeps k ms before copying it, and the fill returns without waiting for
 *     it: a straggler that writes the start of the piece k ms later, every time; out[10] of bpmf_host_call_stats)
 *   svdwf.max_sweeps (60, 1 .. 1000: Jacobi sweeps of bpmf_svdwf_stack_dev before a channel is reported as not
 *     converged; a converged channel is the same at any cap -- the tests pass 1 to reach that status)
 *   mf.split16 (off by default; CHANGES RESULTS within a stated tolerance: matched-filter numerators on the fp16
 *     matrix pipe from hi/lo splits of data and templates, three products, fp32 accumulation -- csrc/mf_split.h;
 *     |d cc_sum| <= 3e-7 * sum|w| measured, 2e-5 allowed by the north star; against its float64 definition: bit-equal
 *     to the exact path where the split is exact, rms error 0.8-2.3 x the exact path's own elsewhere;
 *     x 2.3-2.4 at configs[1]; TEMPLATES OF UP TO 2049 SAMPLES -- the one statement of that limit: it is the MFMA kernels' own (mf_choose in csrc/mf.hip: 4096
 *     lags + the padded template within 24 staging registers of 256 threads), correlated in segments of at most 376
 *     samples; a longer template runs the exact generic kernel, bit-identical to the oracle
 *     (tests/test_gpu_split16_anchor.py pins both sides); composes with the mf.compat_* switches; 1 leaves launches of fewer
 *     than 128 (template, 8192-lag block) pairs to the exact kernel (latency-bound there), 2 takes every launch; enlarges
 *     bpmf_mf_workspace_bytes and what a prepared day holds: set it before the day's first call; does NOT apply to full
 *     normalisation: a launch with BPMF_MF_NORMALIZE_FULL takes family 0, 1 or 2 whatever this option says;
 *     NON-FINITE SAMPLES: the power-of-two scale of a data or template channel comes from its largest FINITE magnitude, so
 *     a NaN or +-Inf costs what it costs the exact path (below, "Non-finite samples") with a reach of
 *     16 * nks + (n_seg - 1) * seg - L - (moveout mod 8) samples: at most 40 for L = 200 or 400, 64 for L = 800; finite
 *     channels and lags in front of that reach keep the bits they have without the bad sample; never +-Inf)
 *   and the result-changing upstream-compatibility switches (off by default; every one has
 *   a variant of the CPU oracle and tools/diff_upstream.py tells which combination equals the real packages):
 *   mf.compat_exclusive_last_lag mf.compat_sqrt_norm mf.compat_range_all_channels mf.compat_sequential_csum
 *   bp.compat_first_computed bp.compat_strict_upper_only bp.compat_range_all_stations
 * (The reference's counterpart is the `device=` / `arch=` string it forwards to the third-party
 * back-ends, BPMF/similarity_search.py:532, BPMF/template_search.py:554.)
 * -1 for an unknown name or a value outside the option's range. */
int bpmf_set_option(const char *name, long value);
int bpmf_get_option(const char *name, long *value, long *default_value);

/* ------------------------------------------------------------ matched filter --- */
/*
 * Serves fast_matched_filter.matched_filter(templates, moveouts, weights, data, step,
 * arch="gpu", network_sum=...) as called at BPMF/similarity_search.py:526-533 and
 * BPMF/dataset.py:4818-4827.
 *   templates (T,S,C,L) f32   moveouts (T,S,C) i32   weights (T,S,C) f32
 *   data (S,C,N) f32          n_corr = (N-L)/step + 1
 *   network_sum != 0 -> cc_out (T, n_corr)          weighted network sum
 *   network_sum == 0 -> cc_out (T, n_corr, S, C)    per-channel CC (unweighted)
 *
 * Non-finite samples (tests/nonfinite_cases.py is the rule in NumPy).  The window norms come from a
 * prefix sum of data^2, so per channel, for the window [j, j + L) of a lag:
 *   +0   a window that holds a NaN; every window that starts behind the channel's first NaN or +-Inf (the rest of
 *        the day: the norm is NaN and the guard r_t * r_d < 1000 fails); every lag of a template channel that holds a NaN
 *   NaN  a window that holds +-Inf and no NaN and does not start behind an earlier bad sample (norm 0, cc = num * 0);
 *        a template channel that holds +-Inf, wherever the window norm is a finite number
 *   0 or NaN  a window that holds a finite sample whose square overflows float32 (NaN where the numerator overflows)
 *   the value it has with the bad samples replaced by +0, bit for bit: every window that ends more than R samples in
 *        front of the channel's first bad sample, and every channel that holds none
 *   that value or NaN: a window that ends within R samples in front of a NaN or +-Inf -- the MFMA kernels multiply the
 *        zeros of their band with those samples.  R = 0 for the generic kernel (family 0), 16 * ceil((L + 15) / 16) - L
 *        (15 .. 30) for the wave and workgroup kernels (families 1, 2), see option mf.split16 for family 3.
 * A channel that is +0 costs the network sum nothing, one that is NaN makes the lag NaN (the caller scrubs NaN:
 * BPMF/similarity_search.py:540).  No output is ever +-Inf.  With BPMF_MF_NORMALIZE_FULL every class above is +0
 * except the last two (Inf - Inf in the centred energy; t - mean t for a template); the channel constant is taken
 * over the finite samples, so the windows in front of a bad sample stay what they are without it.
 */

/* flags of bpmf_mf_run_dev */
#define BPMF_MF_DATA_PREPARED 1 /* workspace already holds this data's window energies */
#define BPMF_MF_FORCE_DIRECT 2  /* use the generic (non-MFMA) kernel */
/* Full normalisation (fast_matched_filter's normalize="full"): the window mean is removed, every per-channel value is
 * the Pearson correlation
 *   cc = sum (t - mean t)(x - mean x) / sqrt(sum (t - mean t)^2 * sum (x - mean x)^2),
 * exactly +0 for a window of L equal samples (a zero- or constant-filled gap; every window when L = 1), for a flat
 * template channel, and under the energy guard on the centred energies.  Lag ranges, weights, the network sum and
 * network_sum == 0 are those of short mode.  A flag of bpmf_mf_run_dev, bpmf_mf_run, bpmf_mf_run_multi and
 * bpmf_mf_launch_info.  The three main kernels are short mode's, run on a centred copy of the day and of the templates
 * (csrc/mf_full.hip): the workspace is bpmf_mf_full_workspace_bytes, the per-day preparation
 * bpmf_mf_prepare_data_full_dev.  BPMF_MF_DATA_PREPARED is accepted only on a workspace whose day was prepared for the
 * same normalisation: with this flag on a day prepared by bpmf_mf_prepare_data_dev (or on another day), or without it on
 * a day prepared by bpmf_mf_prepare_data_full_dev, the call fails with status -1.  Composes with
 * mf.compat_exclusive_last_lag and mf.compat_range_all_channels; NOT defined under mf.compat_sqrt_norm or
 * mf.compat_sequential_csum: every call with the flag then fails with status -1, bpmf_mf_launch_info included.
 * Option mf.split16 does NOT apply: a launch with this flag takes family 0, 1 or 2 whatever that option says.
 * The host-pointer calls upload the day whole before preparing it (the constant a channel is centred by is its mean
 * over the whole day): mf.host_piece_lags has no effect there. */
#define BPMF_MF_NORMALIZE_FULL 4

size_t bpmf_mf_workspace_bytes(size_t L, size_t N, size_t T, size_t S, size_t C);
/* The workspace of a call with BPMF_MF_NORMALIZE_FULL: the short-mode per-day arrays, then the centred day, a second
 * prefix array and the flatness count (all per day, in front of everything that depends on T), then the per-batch
 * arrays and the centred templates.  Independent of mf.split16. */
size_t bpmf_mf_full_workspace_bytes(size_t L, size_t N, size_t T, size_t S, size_t C);

/* Per-day, template-independent preparation (window energies of `data` for length L).
 * Implied by bpmf_mf_run_dev unless BPMF_MF_DATA_PREPARED is set. */
int bpmf_mf_prepare_data_dev(const float *d_data, size_t L, size_t N, size_t S, size_t C,
                             void *d_workspace, size_t workspace_bytes, bpmf_stream_t stream);

/* The same for BPMF_MF_NORMALIZE_FULL (a workspace of bpmf_mf_full_workspace_bytes): per channel the constant
 * c = float32((float64 sum of the FINITE samples) / N) -- the float64 mean of a finite channel, 0 when no sample is
 * finite; a NaN or +-Inf sample does not reach it --, d' = d - c, double prefix sums of d' and d'^2, the reciprocal norms of the centred window
 * energies Q - P * P / L, +Inf for a window of L equal samples (decided from sample equality, not from the energy). */
int bpmf_mf_prepare_data_full_dev(const float *d_data, size_t L, size_t N, size_t S, size_t C,
                                  void *d_workspace, size_t workspace_bytes, bpmf_stream_t stream);

int bpmf_mf_run_dev(const float *d_templates, const int32_t *d_moveouts,
                    const float *d_weights, const float *d_data, size_t step, size_t L,
                    size_t N, size_t T, size_t S, size_t C, size_t n_corr, int network_sum,
                    int flags, void *d_workspace, size_t workspace_bytes,
                    bpmf_stream_t stream, float *d_cc_out);

/* Which kernel a bpmf_mf_run_dev launch of these sizes takes under the current options, and how: every
 * matched-filter kernel family gives the same bits, so this is the only way to see which one runs (the tests
 * assert it wherever they set an option to reach a family; the counterpart of bpmf_bp_plan_info).  Needs no
 * device, workspace or stream.  out[BPMF_MF_LAUNCH_INFO_FIELDS]:
 *   [0] family: 0 generic (direct) kernel, 1 workgroup MFMA kernel, 2 wave MFMA kernel, 3 mf.split16
 *   [1] [2] staging registers per thread of the compiled MFMA variant (window, band); 0 for families 0 and 3
 *   [3] tiles of 256 lags per wave (family 2)      [4] per-template preparation fused into the kernel
 *   [5] channels split over four waves             [6] mf.compat_sqrt_norm epilogue    [7] step == 1
 *   [8] mf_prologue_kernel runs in front           [9] lags per workgroup
 *   [10] dynamic LDS bytes (families 1, 2)         [11] workgroups of the launch
 *   [12] refusal: 0 none, 1 "grid too large", 2 "at most 65535 templates" (bpmf_mf_run_dev fails with it) */
#define BPMF_MF_LAUNCH_INFO_FIELDS 13
int bpmf_mf_launch_info(size_t step, size_t L, size_t N, size_t T, size_t S, size_t C, size_t n_corr,
                        int network_sum, int flags, int64_t *out);

int bpmf_mf_run(const float *templates, const int32_t *moveouts, const float *weights,
                const float *data, size_t step, size_t L, size_t N, size_t T, size_t S,
                size_t C, size_t n_corr, int network_sum, int flags, int device,
                float *cc_out);

/* The same call with the templates block-partitioned over several GPUs inside the library
 * (one host thread per distinct device, every device holds the whole `data`): what upstream's
 * `arch="gpu"` back-end does with every visible device.  The data reach the first device from the
 * host once and the others device -> device (option multi.peer_fanout; upstream copies the day to
 * every device from the host); no CC value crosses devices.
 *   n_devices <= 0: all visible devices; devices == NULL: devices 0 .. n_devices-1. */
int bpmf_mf_run_multi(const float *templates, const int32_t *moveouts, const float *weights,
                      const float *data, size_t step, size_t L, size_t N, size_t T, size_t S,
                      size_t C, size_t n_corr, int network_sum, int flags, int n_devices,
                      const int *devices, float *cc_out);

/* The template ranges of that split: block r computes templates [bounds_out[r], bounds_out[r+1]),
 * balanced by the number of channels with a non-zero weight (the kernels skip the others) -- the
 * same rule as seismic_bpmf_amd.parallel.shard_bounds_weighted, which the torch.distributed path
 * uses.  Pure host function (no device needed); bounds_out has n_blocks + 1 entries. */
int bpmf_mf_shard_bounds(const float *weights, size_t T, size_t S, size_t C, size_t n_blocks,
                         size_t *bounds_out);

/* ------------------------------------------------------------ backprojection --- */
/*
 * Serves beampower.beampower.beamform(waveform_features, moveouts, weights_phases,
 * weights_sources, device="gpu", out_of_bounds=, reduce=) as called at
 * BPMF/template_search.py:549-558 (reduce="max") and :560-569 (reduce="none").
 *   features (S,C,N) f32     moveouts (K,S,P) i32 (samples)
 *   w_phases (S,C,P) f32     w_sources (K,S) f32
 *   reduce max  -> beam_out (N) f32 + arg_out (N) i32   (lowest source index on ties)
 *   reduce none -> beam_out (K,N) f32, arg_out unused (may be NULL)
 */
#define BPMF_BP_STRICT 0
#define BPMF_BP_FLEXIBLE 1
#define BPMF_BP_REDUCE_MAX 0
#define BPMF_BP_REDUCE_NONE 1

typedef struct bpmf_bp_plan bpmf_bp_plan; /* opaque: device-resident moveout table */

/* Build the device-resident plan of one moveout table + source weights (host arrays).
 * The reference rebuilds this table on every access (template_search.py:444-454); the
 * plan is what lets it stay resident across days.  `source_id_offset` is added to the
 * arg-max indices (global ids when the grid is sharded across GPUs). */
int bpmf_bp_plan_create(const int32_t *moveouts, const float *w_sources, size_t K, size_t S,
                        size_t P, int device, int32_t source_id_offset, bpmf_bp_plan **plan);
void bpmf_bp_plan_destroy(bpmf_bp_plan *plan);

/* Shape of a plan (diagnostics; bench.py prices the LDS roofline of the gather width in use). */
typedef struct {
    int32_t n_groups;      /* groups of sources that share one set of LDS windows */
    int32_t tile;          /* time samples per workgroup */
    int32_t lds_bytes;     /* LDS of the largest group */
    int32_t gather_bytes;  /* 8: dual (shifted) windows + ds_read_b64 gathers; 4: 4-byte gathers */
    int32_t stations_max;  /* padded station slots per source of the packed kernel (0: generic kernel) */
    int32_t waves_per_cu;  /* resident waves per CU of the beam kernel this plan dispatches to */
    /* reduce="max": the interior tiles of a two-phase grid run the 8-byte-gather kernel once per
     * station-count class of sources (<= 16, 17..32, 33..64 weighted stations), each class on the
     * largest tile (512 / 256 / 128 samples) at which its dual windows fit the LDS.  0 classes: the
     * general kernels compute everything.  With classes, tile / n_groups / lds_bytes above describe
     * the class that holds most sources. */
    int32_t n_classes;
    int32_t class_tile[3], class_sources[3], class_groups[3], class_stations_max[3];
} bpmf_bp_plan_stats;
int bpmf_bp_plan_info(const bpmf_bp_plan *plan, bpmf_bp_plan_stats *out);

size_t bpmf_bp_workspace_bytes(const bpmf_bp_plan *plan, size_t N, size_t C);

/* The plan that bpmf_bp_plan_create would build from these host tables under the current options, and the schedule
 * of one run on it: the host side of planning alone (the counterpart of bpmf_mf_launch_info).  Needs no device,
 * workspace or stream.  n_events = 0: one series of N samples as bpmf_bp_run_dev runs it with this `reduce`;
 * n_events = E >= 1: a batch of E series as bpmf_bp_relocate_batch_dev runs their max-beams (reduce max only).
 * out[BPMF_BP_LAUNCH_INFO_FIELDS]:
 *   the plan
 *   [0] K  [1] S  [2] P         [3] samples per thread of the general kernels (tile = 256 x it; 4 without LDS plan)
 *   [4] padded (station, phase) terms per source    [5] padded stations of the packed records (P = 2), or 0
 *   [6] padded terms of the per-term table, or 0    [7] dual (shifted) windows    [8] groups  [9] LDS bytes of the largest
 *   [10] 0: an LDS plan; else why the grid takes bp_direct.hip: 1 a source's windows exceed the LDS, 2 more than 256
 *        terms per source, 3 option bp.direct, 4 option bp.compat_strict_upper_only and a negative used moveout
 *   [11] interior-tile classes in use   [12] the one class doubles as the general kernels' plan   [13] classes
 *   [14 + 7 c ...] class c = 0..2: tile, multi-residency groups, residencies per group, group entries, LDS bytes,
 *        sources, most weighted stations of a source
 *   [35] [36] smallest and largest used moveout     [37] source id offset (0)
 *   the schedule
 *   [38] path: 0 bp_direct.hip, 1 class kernels on the interior samples [lo_s, hi_s) + the general kernel on the edge
 *        samples, 2 the general kernel on every sample
 *   [39] general kernel: 0 none (path 0), 1 packed records (bp_beam_wps2_kernel), 2 per-term table
 *        (bp_beam_wps_kernel), 3 bp_beam_kernel;  its template arguments: [40] waves per workgroup [41] stations
 *        [42] 8-byte gathers (family 1), [43] terms (family 2), [44] samples per thread [45] blocks of 64 terms (family 3)
 *   [46] its samples per workgroup  [47] dynamic LDS bytes  [48] resident waves per CU  [49] bytes per gather
 *   [50] group ranges per tile (path 1: of every class kernel; path 0: source ranges)  [51] ... of the general kernel
 *        on the edge samples
 *   [52] partial (beam, arg) rows per series; 1: the kernels write the outputs themselves, no merge launch
 *   [53] lo_s  [54] hi_s (both 0 unless path 1)
 *   [55] [56] [57] byte offsets in the workspace of the prestack(s), the partial beam rows and the partial arg rows
 *        ([56] = [57] when [52] is 1)              [58] bytes of the workspace up to the end of the partial rows:
 *        bpmf_bp_workspace_bytes for n_events = 0 (sized for either `reduce`)
 *   [59 ... 77] what bpmf_bp_plan_info reports of the plan: n_groups, tile, lds_bytes, gather_bytes, stations_max,
 *        waves_per_cu, n_classes, class_tile[3], class_sources[3], class_groups[3], class_stations_max[3] */
#define BPMF_BP_LAUNCH_INFO_FIELDS 78
int bpmf_bp_launch_info(const int32_t *moveouts, const float *w_sources, size_t K, size_t S, size_t P,
                        size_t N, int reduce, size_t n_events, int64_t *out);

/* Non-finite features (DESIGN.md s4 "Non-finite features"): a beam is NaN / +-Inf exactly as IEEE makes the oracle's
 * sum (a zero-weight station, a dropped flexible term and a strict beam that is not computed cost nothing); under
 * reduce max a NaN beam is never the maximum, +Inf is (lowest source id), -Inf never beats the (0, id_offset) floor
 * and d_beam_out is never NaN. */
int bpmf_bp_run_dev(const bpmf_bp_plan *plan, const float *d_features,
                    const float *d_w_phases, size_t N, size_t C, int out_of_bounds,
                    int reduce, void *d_workspace, size_t workspace_bytes,
                    bpmf_stream_t stream, float *d_beam_out, int32_t *d_arg_out);

int bpmf_bp_run(const float *features, const int32_t *moveouts, const float *w_phases,
                const float *w_sources, size_t N, size_t K, size_t S, size_t C, size_t P,
                int out_of_bounds, int reduce, int device, float *beam_out, int32_t *arg_out);

/* The same call with the source grid block-partitioned over several GPUs inside the library.
 * reduce max: the per-device maxima are merged on the host in ascending block order with a
 * strict >, so ties keep the lowest source index exactly like one sequential scan;
 * reduce none: every device fills its own rows of beam_out.  n_devices / devices as above; the
 * features reach the devices like the data of bpmf_mf_run_multi (option multi.peer_fanout). */
int bpmf_bp_run_multi(const float *features, const int32_t *moveouts, const float *w_phases,
                      const float *w_sources, size_t N, size_t K, size_t S, size_t C, size_t P,
                      int out_of_bounds, int reduce, int n_devices, const int *devices,
                      float *beam_out, int32_t *arg_out);

/* The beamforming step of Event.relocate_beam (BPMF/dataset.py:2186-2245; tutorial notebook 6 loops it over every
 * detected event) for a BATCH of E events on one resident plan (bp_relocate.hip).  Every event is a short feature
 * array of N samples (60-120 s); per event the call finds the point of maximum focusing of its (K, N) beam volume --
 * np.unravel_index(beam.argmax(), beam.shape): the first maximum in source-major order -- WITHOUT making the volume:
 * prestack and max-beam of all events in shared launches (the general beam kernels over an event dimension), one
 * focus launch, and for BPMF_BP_RELOCATE_SPATIAL the beam column beam[:, time_idx] of every event, gathered in the
 * oracle's order, and Beamformer._likelihood of it (BPMF/template_search.py:498-506):
 * ((col - min) / (max - min)).clip(0, 1) in float32, NaN for a constant column.  BPMF_BP_RELOCATE_TEMPORAL
 * (reduce="max", dataset.py:2217-2231) returns the max-beam rows, time_idx = first maximum of a row.
 *   element (e, s, c, t) of the features is d_features[e * event_stride + d_starts[e] + (s C + c) row_stride + t]:
 *     one array per event   (E, S, C, N):  event_stride = S C N, row_stride = N, d_starts = NULL;
 *     windows of a day      (S, C, N_day): event_stride = 0, row_stride = N_day, d_starts (E) i64 first samples.
 *     A window must lie inside its row; samples outside read as 0 (the Python caller refuses such windows).
 *   d_moveouts (K, S, P) i32, d_w_sources (K, S) f32: the tables the plan was created from, on the device (the plan
 *     keeps them in its LDS-window form only; the column needs them as they are).  Unused (NULL) for TEMPORAL.
 *   d_time_idx, d_src_idx (E) i32, d_max_beam (E) f32: sample, source id (plan's source_id_offset included) and
 *     value of the maximum.  The result equals the per-event path (bpmf_bp_run_dev + arg-max) whenever
 *     d_max_beam[e] > 0 or the event's volume is all zero; an event with d_max_beam[e] == 0 and any negative beam
 *     is the caller's to redo one by one (seismic_bpmf_amd.workflow.relocate_events does).
 *   SPATIAL: d_likelihood (E, K) f32; d_columns (E, K) f32 or NULL: the raw beam columns.
 *   TEMPORAL: d_maxbeam (E, N) f32, d_maxbeam_sources (E, N) i32.  Unused pointers may be NULL.
 * E <= 65535 per call: callers chunk (results do not depend on the chunking).  Refused (-1) while a bp.compat_*
 * option is set: focus and column are written for the build's conventions.  A plan without LDS windows
 * (bp_direct.hip) runs its events' max-beams one after the other inside the call; everything else is batched.
 * Workspace: bpmf_bp_relocate_workspace_bytes(plan, E, N, C) bytes -- E prestacks (S P N floats each), the
 * partial rows of the group-range split and, for SPATIAL, the (E, N) max-beam rows.
 * Non-finite features: the focus is taken on the max-beams, so a NaN beam is never the maximum and +Inf is (np.argmax
 * on a volume with a NaN is deliberately not followed); a NaN in the column at the focus makes the whole likelihood
 * row NaN, an Inf maximum gives 0 on the finite entries and NaN at the Inf. */
#define BPMF_BP_RELOCATE_SPATIAL 0
#define BPMF_BP_RELOCATE_TEMPORAL 1
size_t bpmf_bp_relocate_workspace_bytes(const bpmf_bp_plan *plan, size_t E, size_t N, size_t C);
int bpmf_bp_relocate_batch_dev(const bpmf_bp_plan *plan, const float *d_features, size_t event_stride,
                               size_t row_stride, const int64_t *d_starts, const float *d_w_phases,
                               const int32_t *d_moveouts, const float *d_w_sources, size_t E, size_t N, size_t C,
                               int out_of_bounds, int method, void *d_workspace, size_t workspace_bytes,
                               bpmf_stream_t stream, int32_t *d_time_idx, int32_t *d_src_idx, float *d_max_beam,
                               float *d_likelihood, float *d_columns, float *d_maxbeam,
                               int32_t *d_maxbeam_sources);

/* The end of Event.relocate_beam (BPMF/dataset.py:2207-2245) for a chunk of E events that
 * bpmf_bp_relocate_batch_dev has just relocated, on its outputs where they lie (bp_uncertainty.hip): the restricted
 * domain around each new epicentre (Beamformer._rectangular_domain, BPMF/template_search.py:1232-1267), and the
 * likelihood-weighted mean geodesic distance and mean absolute depth difference of the domain's sources
 * (Beamformer._compute_location_uncertainty, :1269-1333).  No host synchronisation; everything on `stream`.
 *   d_src_idx (E) i32: the events' source ids as bpmf_bp_relocate_batch_dev wrote them (the plan's source_id_offset
 *     included; the tables are indexed with id - offset).
 *   d_tables (6, K) f64, one value per source ROW of the plan: longitude, latitude (degrees), depth (km),
 *     dist_per_lat = 2 pi / 360 * 6371 * sin(deg2rad(90 - latitude)), sin and cos of the reduced latitude
 *     atan((1 - f) tan(latitude)) on WGS84.  dist_per_lon = 2 pi / 360 * 6371; half_side_km = side_km / 2.
 *   SPATIAL:  terms are the K sources, weight d_likelihood[e, k] (f32, widened exactly), source k takes part if
 *     |lon_k - lon_0| dist_per_lon < half_side_km and |lat_k - lat_0| dist_per_lat[row_0] < half_side_km, evaluated
 *     as NumPy evaluates it in float64.  d_domain_mask (E, K) u8 or NULL receives the test.
 *   TEMPORAL: terms are the N samples, source d_maxbeam_sources[e, t] - offset, weight
 *     expf(-(d_max_beam[e] - d_maxbeam[e, t]) / (float)effective_kT) in float32; a sample takes part if its weight
 *     is > (float)gibbs_cutoff.  d_domain_mask must be NULL.
 *   Outputs (E): d_hunc = sum w d / sum w, d in km along the WGS84 geodesic (Vincenty's inverse, |d lambda| < 1e-12,
 *     200 iterations at most, pi (a + b) / 2 for a pair that does not converge); d_vunc = sum w |depth_0 - depth| /
 *     sum w; d_n_domain: the terms that took part; d_longitude, d_latitude, d_depth: the event's row of the tables.
 *     sum w = 0 and NaN weights give NaN.  A source id outside the plan gives NaN and d_n_domain = -1.
 *   The numerators are float64 sums in a fixed tree (256 terms per workgroup, then one workgroup per event).  The
 *     denominator is what the reference divides by: np.sum of the float32 weights that take part, a FLOAT32 sum in
 *     NumPy's order (chunks of 8192 added in turn, each summed pairwise), reproduced bit for bit.  The result of an
 *     event does not depend on E, on the chunk or on the run.
 * E <= 65535 per call.  Workspace: bpmf_bp_location_uncertainty_workspace_bytes(E, K or N) bytes. */
size_t bpmf_bp_location_uncertainty_workspace_bytes(size_t E, size_t n_terms);
int bpmf_bp_location_uncertainty_dev(const bpmf_bp_plan *plan, int method, size_t E, size_t N,
                                     const int32_t *d_src_idx, const float *d_likelihood, const float *d_maxbeam,
                                     const int32_t *d_maxbeam_sources, const float *d_max_beam,
                                     const double *d_tables, double dist_per_lon, double half_side_km,
                                     double effective_kT, double gibbs_cutoff, void *d_workspace,
                                     size_t workspace_bytes, bpmf_stream_t stream, double *d_hunc, double *d_vunc,
                                     int32_t *d_n_domain, double *d_longitude, double *d_latitude, double *d_depth,
                                     uint8_t *d_domain_mask);

/* Multi-GPU exchange step of reduce="max": pack (beam, source id) into one uint64 whose
 * unsigned order is (beam ascending, then source id DEscending), so that an RCCL
 * all-reduce with ncclMax over uint64 (or int64 after the bias below) yields the global
 * maximum with the lowest source id on ties; unpack restores the two vectors.
 * `as_signed` != 0 flips the top bit so that the order also holds for int64 (torch has
 * no uint64 reductions). */
int bpmf_bp_pack_max_dev(const float *d_beam, const int32_t *d_arg, size_t N, int as_signed,
                         bpmf_stream_t stream, uint64_t *d_packed);
int bpmf_bp_unpack_max_dev(const uint64_t *d_packed, size_t N, int as_signed,
                           bpmf_stream_t stream, float *d_beam, int32_t *d_arg);

/* ------------------------------------------------------- inter-template CC, batched --- */
/*
 * The core of TemplateGroup.compute_intertemplate_cc (BPMF/dataset.py:4775-4841) for ALL template
 * pairs in one pass (the reference makes one fast_matched_filter call per template, :4818-4827):
 *   out[t, u] = sum_{s,c} base_weights[t, s, c] * max_{lag} CC(trimmed template u, waveform t at lag)
 * for the pairs with pair_mask[t, u] != 0, else 0; trimmed = samples [max_lag, Lw - max_lag),
 * lag = 0 .. 2 max_lag; CC = the matched filter's normalised cross-correlation (zero moveouts),
 * 0 on channels of zero weight; the channel sum runs in NumPy's pairwise order, so the matrix
 * equals the reference's per-template loop bit for bit.  The caller symmetrises ((out + out^T)/2,
 * dataset.py:4833-4834).
 *   d_waveforms (T,S,C,Lw) f32   d_base_weights (T,S,C) f32   d_pair_mask (T,T) u8   d_out (T,T) f32
 * Limits, checked before anything is launched or written (-1, d_out untouched): Lw > 2 max_lag, max_lag <= 31, and
 * 4 (Lw + 8 (2 max_lag + 1) + 8 S C) <= 65536 bytes -- one channel with its CCs against a tile of 8 templates in LDS.
 */
size_t bpmf_intertemplate_workspace_bytes(size_t T, size_t S, size_t C, size_t max_lag);
int bpmf_intertemplate_cc_dev(const float *d_waveforms, const float *d_base_weights,
                              const uint8_t *d_pair_mask, size_t T, size_t S, size_t C, size_t Lw,
                              size_t max_lag, void *d_workspace, size_t workspace_bytes,
                              bpmf_stream_t stream, float *d_out);

/* ------------------------------------------ detection stage behind the beamformer --- */
/*
 * Device version of the two full-length steps of Beamformer.find_detections
 * (BPMF/template_search.py:574-627), so that the (N,) max-beam never leaves HBM:
 *
 * bpmf_bp_window_stats_dev: the per-window statistics of template_search.time_dependent_threshold
 * (BPMF/template_search.py:1418-1487): for q = 1 .. n_windows, window q covers the samples
 * [q*shift, min(n, q*shift + window)); d_median[q] / d_mad[q] receive np.median(window) and
 * np.median(|window - median|) in float32, bit for bit (radix select, no sort).  Both arrays need
 * n_windows + 2 entries; entries 0 and n_windows + 1 (the reference's end fills) are left to the
 * caller.  n_windows = bpmf_bp_num_windows(n, window, shift) = (n - window) / shift + 1.
 *
 * bpmf_bp_extract_peaks_dev: every rising-edge local maximum of the max-beam (the peak rule of
 * utils._detect_peaks, BPMF/utils.py:2292-2301: x[t] - x[t-1] > 0 and x[t+1] - x[t] <= 0 in float64
 * -- x[t] > x[t-1] and x[t+1] <= x[t] on finite values; an isolated +Inf is a peak, a run of equal
 * infinities is none -- first and last sample excluded, samples next to a NaN excluded) whose value
 * exceeds `floor_value` (-Inf: every local maximum; NaN: none), as
 * (sample, beam, source) records in arbitrary order.  *d_count receives the number found (may
 * exceed `capacity`; only the first `capacity` are stored).  d_sources may be NULL (source = 0).
 */
typedef struct bpmf_bp_peak {
    int32_t index;  /* time sample */
    float beam;     /* maxbeam[index] */
    int32_t source; /* maxbeam_sources[index] */
    int32_t pad;
} bpmf_bp_peak;

size_t bpmf_bp_num_windows(size_t n, size_t window, size_t shift);
int bpmf_bp_window_stats_dev(const float *d_beam, size_t n, size_t window, size_t shift,
                             bpmf_stream_t stream, float *d_median, float *d_mad);
int bpmf_bp_extract_peaks_dev(const float *d_beam, const int32_t *d_sources, size_t n,
                              double floor_value, uint32_t capacity, bpmf_stream_t stream,
                              uint32_t *d_count, bpmf_bp_peak *d_records);

/* ------------------------------------------------ post-CC detection threshold --- */
/*
 * Device version of the step right after the matched filter:
 * BPMF.clib.time_dependent_threshold (BPMF/clib.py:257-309 -> BPMF/libc.c:516-673, RMS variant)
 * for ALL rows of a (n_rows, n) CC matrix resident in HBM, and the extraction of the samples above
 * the threshold (BPMF/similarity_search.py:231-232, with the cap of :629), so that only candidate
 * records leave the device.  Results equal the reference's single-threaded libc.c bit for bit.
 *   half_window = window // 2, shift = int((1 - overlap) * window)   (as clib.py:292-293)
 *   gaussian: 500 standard-normal floats used to fill exact zeros (libc.c:606-612)
 *   thr_windows (n_rows, n_win): one threshold per sliding window, after "delay the jump"
 *   threshold (n_rows, n) or NULL: the step-wise expansion the reference returns
 * Limits: 2 * half_window < 2^31, 1 <= shift <= 2 * half_window + 1, n >= 2 * half_window.  With `threshold`
 * (the expansion) n_rows <= 65535 per call (gridDim.y); without it any number of rows goes.  Both extractions
 * below take n_rows <= 65535 and n < 2^31 per call.  A call outside these limits returns -1 before anything
 * is launched or written (bpmf_last_error says why); callers with more rows hand them over in slabs.
 */
size_t bpmf_tdt_num_windows(size_t n, size_t half_window, size_t shift);
size_t bpmf_tdt_workspace_bytes(size_t n_rows, size_t n, size_t half_window, size_t shift);
int bpmf_tdt_rms_dev(const float *d_series, const float *d_gaussian, float num_dev, size_t n_rows,
                     size_t n, size_t half_window, size_t shift, void *d_workspace,
                     size_t workspace_bytes, bpmf_stream_t stream, float *d_thr_windows,
                     float *d_threshold);

typedef struct bpmf_candidate {
    int32_t row;     /* template (row of the CC matrix) */
    int32_t index;   /* CC index (x step = data sample) */
    float cc;        /* CC value */
    float threshold; /* threshold it exceeded */
} bpmf_candidate;

/* Append one record per sample with cc > min(threshold, row_cap[row]) (row_cap may be NULL).
 * *d_count receives the number of candidates found (may exceed `capacity`; only the first
 * `capacity` are stored, in arbitrary order). */
int bpmf_extract_candidates_dev(const float *d_series, const float *d_thr_windows,
                                const float *d_row_cap, size_t n_rows, size_t n,
                                size_t half_window, size_t shift, uint32_t capacity,
                                bpmf_stream_t stream, uint32_t *d_count,
                                bpmf_candidate *d_records);

int bpmf_extract_candidates_mad_dev(const float *d_series, const float *d_thr_windows,
                                    const float *d_row_cap, size_t n_rows, size_t n, size_t window,
                                    size_t shift, uint32_t capacity, bpmf_stream_t stream,
                                    uint32_t *d_count, bpmf_candidate *d_records);

/* The optional validation of MatchedFilter.select_cc_indexes (BPMF/similarity_search.py:253-272) on the device:
 * for detection q, how many samples of row d_rows[q] of the (n_rows, n) matrix lie strictly below d_level[q] in
 * [d_start[q], d_start[q] + d_len_left[q]) -> d_below[2 q] and in the d_len_right[q] samples behind -> d_below[2 q + 1]
 * (float32 compares, like the reference's `cc1 < cc_at_mean_plus_1sig[cc_idx[i]]`; one workgroup per detection; a
 * few thousand detections of a few hundred samples each: the CC rows stay in HBM).  The host keeps a detection when
 * min(below_left / len_left, below_right / len_right) >= anomalous_cdf_at_mean_plus_1sig. */
int bpmf_count_below_dev(const float *d_series, size_t n_rows, size_t n, size_t n_detections,
                         const int32_t *d_rows, const int64_t *d_start, const int32_t *d_len_left,
                         const int32_t *d_len_right, const float *d_level, bpmf_stream_t stream,
                         int32_t *d_below);

/* The peak amplitudes MatchedFilter._find_detections_t attaches to its events (BPMF/similarity_search.py:695-714,
 * `extract_peak_amplitudes`, the reference's default; the input of the magnitude step), gathered from the day of data
 * in HBM (peak_amp.hip): for detection q = (template row d_rows[q], DATA sample d_samples[q] = cc index x step) and
 * channel (s, c)
 *     i1 = d_samples[q] + d_moveouts[row, s, c] - offset;   i2 = i1 + duration;
 *     d_out[q, s, c] = max(data[s, c, i1:i2]) * d_norm[s, c]      (0.0 for an empty slice)
 * with the slice taken as NumPy takes it -- the reference does not guard it: i1 and i2 each get N added when
 * negative and are then clipped to [0, N], so a window that straddles sample 0 is empty, a window wholly before
 * sample 0 wraps to the end of the day, and a window past N is clipped.  A window that holds a NaN gives NaN
 * (np.max); the product is one float32 multiply, and without d_norm the maximum is stored as it is.
 *   d_data (S, C, N) f32; d_rows (n) i32; d_samples (n) i64; d_moveouts (T, S, C) i32 samples (any sign);
 *   d_norm_or_null (S, C) f32; d_out (n, S, C) f32 -- every element is written.
 * Returns -1 for a null pointer, S * C == 0, N, |offset| or |duration| above 2^40, or a row outside [0, T): the rows
 * are checked on the host (a copy of 4 n bytes and one synchronisation of `stream`) before anything is launched.
 * n_detections == 0 launches nothing and returns 0. */
int bpmf_peak_amplitudes_dev(const float *d_data, size_t S, size_t C, size_t N, size_t n_detections,
                             const int32_t *d_rows, const int64_t *d_samples, const int32_t *d_moveouts, size_t T,
                             int64_t offset, int64_t duration, const float *d_norm_or_null, bpmf_stream_t stream,
                             float *d_out);

/* Matched-filter templates cut from the located events of a day that is in HBM (templates.hip; the reference:
 * Event.read_waveforms(time_shifted=True) + set_availability + TemplateGroup.normalize + Event.compute_snr,
 * BPMF/dataset.py:1929-2069, 2556-2607, 4152-4166, 1441-1475).  For event e and channel (s, c), with
 * i0 = d_origin[e] + d_moveouts[e, s, c] and window[l] = data[s, c, i0 + l] where 0 <= i0 + l < N, else +0.0:
 *     d_norm[e, s, c]         = np.std(window) (normalize 1) | np.max(np.abs(window)) (2) | 1 (0);   0 becomes 1
 *     d_templates[e, s, c, l] = window[l] / d_norm[e, s, c]
 *     d_flags[e, s, c]        = bit 0: any(window != 0) (a NaN counts);  bit 1: the window lies wholly inside [0, N)
 *     d_snr[e, s, c]          = np.std(window) / np.std(noise window), a noise std of 0 taken as 1; the noise window
 *                               is the noise_samples samples from d_origin[e] - noise_offset, the same for every
 *                               channel, clipped in place like the signal window
 * in NumPy's own float32 arithmetic (pairwise sums, mean, squared deviations, one division, one square root), so
 * the results equal postprocess.templates_from_events_host bit for bit; a window that holds a NaN gets a NaN norm.
 * A window cut by the START of the day keeps its alignment here (zeros in front); the reference left-aligns what
 * it could read.
 *   d_data (S, C, N) f32; d_origin (E) i64; d_moveouts (E, S, C) i32 WINDOW moveouts in samples (any sign);
 *   d_templates (E, S, C, n_samples) f32; d_norm (E, S, C) f32; d_flags (E, S, C) u8; d_snr_or_null (E, S, C) f32,
 *   given exactly when noise_samples > 0.  Every element of every output is written.
 * Returns -1 for a null pointer, n_samples == 0 or > 8192, noise_samples > 8192 (NumPy sums longer rows in
 * buffers of 8192 samples: another summation tree), normalize outside 0..2, S * C == 0, N == 0, E * S * C >= 2^31,
 * N or |noise_offset| above 2^40, d_snr without noise_samples or the reverse, or an origin beyond +-2^40: the
 * origins are checked on the host (a copy of 8 E bytes and one synchronisation of `stream`) before anything is
 * launched.  n_events == 0 launches nothing and returns 0. */
int bpmf_templates_from_events_dev(const float *d_data, size_t S, size_t C, size_t N, size_t n_events,
                                   const int64_t *d_origin, const int32_t *d_moveouts, size_t n_samples,
                                   int normalize, int64_t noise_offset, size_t noise_samples, bpmf_stream_t stream,
                                   float *d_templates, float *d_norm, uint8_t *d_flags, float *d_snr_or_null);

/* The running Z-score in front of the deep-learning phase picker (picker.hip; the reference: utils.normalize_batch,
 * BPMF/utils.py:1966-2036, called on every event by Event.pick_PS_phases, BPMF/dataset.py:1706-1927, through the
 * ml_picker of tutorial/notebooks/6_relocate.ipynb).  Row (r, c), r < n_rows, c < C, is
 *     x[i] = d_data[r % S, c, d_start[r] + i] where 0 <= d_start[r] + i < N, else +0.0        (i = 0 .. n_samples-1)
 * -- the windows of E events x S stations of a day in HBM (n_rows = E * S), or an already cut (R, C, n) tensor
 * (S = n_rows, N = n_samples, d_start_or_null NULL: every start 0).  Each row is reflect-padded by `shift`; the
 * float32 np.mean / np.std of its windows of `window` samples at the multiples of `shift` (a trailing partial window
 * dropped; the first window takes the second's statistics and the last the last but one's; std 0 becomes 1) are
 * interpolated in float64 to every sample from the n_windows abscissae d_nodes as np.interp does, and
 *     d_out[r, c, i] = ((double) x[i] - mean(i)) / std(i)
 * is stored as float64 (out_f64 != 0) or as its (float).  The results equal postprocess.normalize_batch_host bit for
 * bit (NaN samples included; infinite samples are out of scope).  shift = int((1 - overlap) * window) and
 * d_nodes = np.linspace(shift, n_samples - shift, n_windows) are the caller's (postprocess.normalize_batch_plan).
 *   d_data (S, C, N) f32; d_start_or_null (n_rows) i64, clamped to +-2^40; d_nodes (n_windows) f64;
 *   d_out (n_rows, C, n_samples) f32 or f64.  Every element of the output is written.
 * Returns -1 for a null pointer, S * C == 0, N == 0 or above 2^40, n_rows * C >= 2^31, window < 2 or > 8192 (the
 * length NumPy sums in one pairwise tree), shift < 1 or > n_samples - 1, fewer than 2 windows, n_windows other than
 * (n_samples + 2 shift - window) / shift + 1, or a row that does not fit in LDS:
 * n_samples + 2 shift + window + 2 n_windows must be at most 38400 floats (n_samples = 16384 with window = 3000 and
 * shift = 1500 takes 22406).  n_rows == 0 launches nothing and returns 0. */
int bpmf_normalize_batch_dev(const float *d_data, size_t S, size_t C, size_t N, size_t n_rows,
                             const int64_t *d_start_or_null, size_t n_samples, size_t window, size_t shift,
                             const double *d_nodes, size_t n_windows, int out_f64, bpmf_stream_t stream, void *d_out);

/* Polyphase resampling of float32 rows (resample.hip; the reference: scipy.signal.resample_poly(data_arr, upsampling,
 * downsampling, axis=-1) between the cut windows and the picker in Event.pick_PS_phases, BPMF/dataset.py:1801-1804,
 * and Stack.pick_PS_phases_family_mode, :5596-5599).  Rows are addressed as bpmf_normalize_batch_dev addresses them:
 * row (r, c), r < n_rows, c < C, is
 *     x[i] = d_data[r % S, c, d_start[r] + i] where 0 <= d_start[r] + i < N, else +0.0            (i = 0 .. n_in-1)
 * -- windows cut from a day in HBM, or an already cut tensor (S = n_rows, N = n_in, d_start_or_null NULL).  The window
 * is cut FIRST: the samples of the day beside it do not enter.  `up` and `down` are reduced by their gcd; d_table,
 * taps_per_phase (hp) and n_pre_remove are the plan of postprocess.resample_poly_plan: the Kaiser-windowed filter
 * firwin(20 max(up, down) + 1, 1 / max(up, down), ("kaiser", 5.0)) as float32 times up, with the zeros upfirdn runs it
 * with in front and behind, zero-extended to hp taps for each of the `up` phases.  With m = q + n_pre_remove,
 * j_hi = m down / up and t = m down % up,
 *     d_out[r, c, q] = the float32 sum over k = hp - 1 .. 0 of x[j_hi - k] * d_table[t + k up]   (0 <= j_hi - k < n_in)
 * from +0, input index ascending, one rounded multiply and one rounded add per tap (never a fused multiply-add), the
 * zero taps of the padding included (they spread a NaN sample as far as SciPy spreads it).  The results equal
 * postprocess.resample_poly_host, and through it SciPy, bit for bit.  One workgroup per (row, tile of outputs):
 * bpmf_resample_poly_tile(up, down, taps_per_phase) is the tile the host picks (a multiple of 64, at most 1024, so
 * that the table and the tile's input span take at most 48 KB of LDS; 0 for arguments the call below refuses).
 *   d_data (S, C, N) f32; d_start_or_null (n_rows) i64, clamped to +-2^40; d_table (taps_per_phase * up) f32;
 *   d_out (n_rows, C, n_out) f32.  Every element of the output is written.
 * Returns -1, before anything is launched, for a null pointer, S * C == 0, N == 0 or above 2^40,
 * n_rows * C >= 2^31, up or down under 1 or over 64, not reduced, or both 1 (a copy: the caller's), n_in < 1,
 * n_in * max(up, down) >= 2^40, n_out other than ceil(n_in up / down), taps_per_phase == 0 or a table of more than
 * 2048 taps, n_pre_remove above the table's length, or 2^31 workgroups or more.  n_rows == 0 launches nothing and
 * returns 0. */
size_t bpmf_resample_poly_tile(size_t up, size_t down, size_t taps_per_phase);
int bpmf_resample_poly_dev(const float *d_data, size_t S, size_t C, size_t N, size_t n_rows,
                           const int64_t *d_start_or_null, size_t n_in, size_t up, size_t down, const float *d_table,
                           size_t taps_per_phase, size_t n_pre_remove, size_t n_out, bpmf_stream_t stream,
                           float *d_out);

/* The picks of every probability series the picker returns (picker.hip; the reference: utils.find_picks,
 * BPMF/utils.py:2039-2094, called per station and phase by Event.pick_PS_phases, BPMF/dataset.py:1859-1865):
 * scipy.signal.find_peaks(x, height=threshold, prominence=0.9 * threshold, width=1) -- plateau midpoints that a rise
 * opens and a fall closes, prominence over the whole series, width at half prominence -- and per peak, over the
 * samples int(left_ip) .. int(right_ip),
 *     mean = np.sum(samples * prob) / prob.sum();   std = sqrt(np.sum((samples - mean)^2) / prob.sum())
 * with the first and third sums in float64 and prob.sum() in float32, all in NumPy's pairwise order.  Series t uses
 * threshold_even when t is even and threshold_odd when it is odd: a (.., 2, n) array of P and S probabilities.
 *   d_proba (n_traces, n_samples) f32; d_count (n_traces) i32: the TRUE number of picks of the series;
 *   d_value f32, d_mean f64, d_std f64, d_index i32 (the peak sample), each (n_traces, max_picks), ascending in
 *   time: the first min(count, max_picks) picks; the unused slots hold NaN / -1.  Every element is written.
 * The results equal postprocess.find_picks_host bit for bit.
 * Returns -1 for a null pointer, n_samples == 0 or > 16384 (the series is staged in LDS), max_picks == 0 or > 4096,
 * 2^31 series or more, or a NaN threshold.  n_traces == 0 launches nothing and returns 0. */
int bpmf_find_picks_dev(const float *d_proba, size_t n_traces, size_t n_samples, double threshold_even,
                        double threshold_odd, size_t max_picks, bpmf_stream_t stream, int32_t *d_count,
                        float *d_value, double *d_mean, double *d_std, int32_t *d_index);

/* ------------------------------------------------- robust statistics (stats.hip) --- */
/* np.median and MAD (median of |x - median|, float32 like NumPy) of every row of a (rows, n)
 * device array; skip_zeros != 0: over the samples != 0 only (`a[a != 0]`).  NaN for an empty
 * selection or a row that holds a NaN.  d_n_zero (may be NULL) receives the zeros per row.
 * Serves saturated_envelopes (BPMF/template_search.py:1547-1561). */
int bpmf_row_median_mad_dev(const float *d_x, size_t rows, size_t n, int skip_zeros,
                            bpmf_stream_t stream, float *d_median, float *d_mad, int64_t *d_n_zero);

/* The same with a device workspace of bpmf_row_median_mad_workspace_bytes(rows, n) bytes: rows of at least
 * option stats.row_grid_min_n samples are then read twice by workgroups from all over the chip instead of
 * seven times by one workgroup each (a day-long row: 60 envelopes 9.2 -> under 1 ms); same bits.
 * d_workspace NULL = bpmf_row_median_mad_dev. */
size_t bpmf_row_median_mad_workspace_bytes(size_t rows, size_t n);
int bpmf_row_median_mad_ws_dev(const float *d_x, size_t rows, size_t n, int skip_zeros,
                               void *d_workspace, size_t workspace_bytes, bpmf_stream_t stream,
                               float *d_median, float *d_mad, int64_t *d_n_zero);

/* The element-wise steps of the envelope (BPMF/template_search.py:1598-1617) around the library FFTs, one pass each:
 * d_spectrum (rows, bins) complex128, the rfft of the traces, becomes -i X in place with the DC bin -- and, when the
 * trace length is even, the last (Nyquist) bin -- cleared: its irfft is the Hilbert transform; then
 * d_out[i] = (float) sqrt((double) d_x[i]^2 + d_h[i]^2), float64 arithmetic, over `total` samples.  rows <= 65535. */
int bpmf_hilbert_spectrum_dev(void *d_spectrum, size_t rows, size_t bins, int n_is_even, bpmf_stream_t stream);
int bpmf_envelope_combine_dev(const float *d_x, const double *d_h, size_t total, bpmf_stream_t stream,
                              float *d_out);

/* The last step of saturated_envelopes (BPMF/template_search.py:1562-1572) in one pass over the (rows, n)
 * envelopes: (x - median[row]) / mad[row] in float32, 0 for missing samples (exact zeros) and for rows with
 * dead[row] != 0, capped at `cap` (np.minimum: a NaN stays a NaN).  d_out may be d_x.  rows <= 65535 per call. */
int bpmf_saturate_rows_dev(const float *d_x, const float *d_median, const float *d_mad, const int32_t *d_dead,
                           size_t rows, size_t n, float cap, bpmf_stream_t stream, float *d_out);

/* time_dependent_threshold(time_series, sliding_window, overlap, threshold_type="mad",
 * white_noise) of BPMF/similarity_search.py:1079-1113 for every row of a (rows, n) CC matrix:
 * `window` = sliding_window, `shift` = int((1 - overlap) * sliding_window).  d_thr_windows
 * (rows, n_windows) receives centre + num_dev * deviation after the two neighbour-maximum
 * passes; d_thr_full (rows, n), if not NULL, the threshold of every sample.  Row r replaces its
 * zeros, in order, by white_noise[0 .. n_zeros(r)) * deviation0 + centre0; -1 if a row holds
 * more zeros than n_noise (checked with one small D2H and a stream synchronise when n_noise < n:
 * hand over n values, as the reference draws them, to stay asynchronous).
 * Limits: rows <= 65535 per call (gridDim.y; callers with more rows chunk them -- ThresholdGPU
 * does), n < 2^31.  The workspace holds NO copy of the series (since round 5 the zeros are replaced where the
 * medians read them): per row the zero-rank tables (~n / 32 bytes), the window values, and -- for rows of at
 * least option stats.row_grid_min_n samples -- the buffers the two-read row statistics collect the middle of
 * a row in (~n / 6 bytes + 100 KB); bpmf_tdt_mad_workspace_bytes: ~1 GB for 500 rows of a day at 100 Hz, a few
 * KB per row for short rows.  Bound it by calling with fewer rows at a time. */
size_t bpmf_tdt_mad_num_windows(size_t n, size_t window, size_t shift);
size_t bpmf_tdt_mad_workspace_bytes(size_t rows, size_t n, size_t window, size_t shift);
int bpmf_tdt_mad_dev(const float *d_series, const float *d_white_noise, size_t n_noise,
                     float num_dev, size_t rows, size_t n, size_t window, size_t shift,
                     void *d_workspace, size_t workspace_bytes, bpmf_stream_t stream,
                     float *d_thr_windows, float *d_thr_full, int64_t *d_n_zero);

/* scipy.stats.kurtosis(row) (Fisher, biased: m4 / m2^2 - 3, NaN for a constant row) of every row,
 * float32 with NumPy's pairwise summation order: the `sanity_check` of
 * MatchedFilter._find_detections_t (BPMF/similarity_search.py:633-642).  rows <= 65535 per call. */
size_t bpmf_row_kurtosis_workspace_bytes(size_t rows, size_t n);
int bpmf_row_kurtosis_dev(const float *d_x, size_t rows, size_t n, void *d_workspace,
                          size_t workspace_bytes, bpmf_stream_t stream, float *d_kurtosis);

/* The same sums, handed out before the last expression: d_parts (rows, 3) receives (mean, m2, m4) of every row
 * in float32 (d_kurtosis may be NULL).  Why: SciPy evaluates `m4 / m2**2.0 - 3` on NumPy SCALARS when the input is
 * one series -- which is how BPMF calls it (similarity_search.py:640) -- and a NumPy scalar `**` is the C
 * library's powf, which glibc rounds faithfully but not always correctly (one case in 2500 random rows: 2 ulp in
 * the kurtosis); on an ARRAY the same expression is the correctly rounded square, which is what
 * bpmf_row_kurtosis_dev computes.  A host that wants the reference's very bits finishes the expression with its own
 * NumPy scalars (seismic_bpmf_amd.workflow.row_excess_kurtosis does). */
int bpmf_row_kurtosis_parts_dev(const float *d_x, size_t rows, size_t n, void *d_workspace,
                                size_t workspace_bytes, bpmf_stream_t stream, float *d_kurtosis,
                                float *d_parts);

/* ------------------------------------------- SVD-Wiener stack of a template's detections --- */
/*
 * EventGroup.SVDWF_stack (BPMF/dataset.py:4275-4374: utils.SVDWF, BPMF/utils.py:667-772, and utils.bandpass_filter,
 * :24-90, on every channel, then the normalised mean) for a ragged batch of G groups (templates) in one call
 * (svdwf.hip).  Group g holds the events offsets[g] .. offsets[g + 1] of d_x; a channel (g, s, c) is the (n, m) matrix
 * A = d_x[offsets[g] .. offsets[g + 1], s, c, :], w = wiener_colsize, or n where that is 0.  In float64 throughout:
 *   1. the eigenpairs of the Gram matrix on the smaller side (A A^T for n <= m, else A^T A) by two-sided cyclic
 *      Jacobi, one workgroup per channel; sigma_j^2 are its eigenvalues, var = cumsum(sigma^2) / sum(sigma^2);
 *      sum == 0: the channel's output is zeros, k = 0, no band-pass; else
 *      k = min(max_singular_values, 1 + first j with var[j] >= expl_var);
 *   2. for j < k the projection P_j = sigma_j u_j v_j^T, left as it is for w == 1, else scipy.signal.wiener(P_j,
 *      [w, 1]): the local sums of row i run over the rows i - w / 2 .. i + (w - 1) / 2 that exist, divided by w;
 *      noise = the mean local variance of the matrix; where the local variance is below it the local mean, else
 *      (P - mean) (1 - noise / var) + mean.  A projection whose filtered form holds a NaN is skipped whole;
 *   3. their sum, through the same filter once more (w != 1); NaN and +-Inf become 0;
 *   4. with d_sos: every row loses its mean and its least-squares line, is multiplied by tukey(m, taper_alpha) and
 *      goes through the cascade forward and backward (see bpmf_bandpass_rows_dev);
 *   5. d_filtered = (float) of that; d_stack[g, s, c, :] = the float64 mean over the group's events of the float32
 *      values, divided by its signed maximum over the samples (a maximum of 0 divides by 1), as float32.
 * The definitions are seismic_bpmf_amd.postprocess.svdwf_host / svdwf_stack_host; the device is within 2^-22 of the
 * channel's largest |filtered| and 2^-21 on the stack wherever the retained sigma_j^2 are separated from the next by
 * 1e-4 sigma_1^2.  A channel gives the same bits in any batch and with any workspace.
 *   d_x (N, S, C, m) f32, N = offsets[G]; offsets (G + 1) i64 ON THE HOST, ascending from 0; d_sos_or_null
 *   (n_sections, 6) f64 rows [b0, b1, b2, 1, a1, a2] on the device, NULL: no band-pass; d_filtered_or_null (N, S, C, m)
 *   f32; d_stack (G, S, C, m) f32; d_n_singular (G, S, C) i32 = k; d_status (G, S, C) i32: 0, or 1 where the solver
 *   had not converged after option svdwf.max_sweeps sweeps (that channel's outputs are zeros, k = 0).
 * Every element of every output is written.  An empty group has a zero stack, k = 0 and status 0.
 * The workspace holds the offsets and one slot per channel in flight (two Gram-sized matrices, two (n, m) float64
 * tables, the vectors): bpmf_svdwf_workspace_bytes(G, largest group, m, channels) for `channels` slots; the call
 * processes the G * S * C channels in as many slabs as the slots it is given require (at most 65535 per slab), and
 * needs at least one.  bpmf_svdwf_workspace_bytes returns 0 for sizes that the call refuses.
 * Synchronises `stream` once before the first launch (the offsets are copied to the device).
 * Returns -1 for a null pointer, S * C == 0, n_samples == 0, a group with min(n, m) > 512 or max(n, m) > 16384,
 * max_singular_values outside 1 .. 8, expl_var outside (0, 1], wiener_colsize > 65536, d_sos with 0 or more than 8
 * sections or a taper_alpha that is NaN, offsets that do not start at 0 or do not ascend, N * S * C or
 * G * S * C >= 2^31, or a workspace smaller than the offsets and one slot (the offsets alone where every group is
 * empty).  G == 0 launches nothing and returns 0.
 */
size_t bpmf_svdwf_workspace_bytes(size_t n_groups, size_t max_group_size, size_t n_samples, size_t n_channels);
int bpmf_svdwf_stack_dev(const float *d_x, const int64_t *offsets, size_t n_groups, size_t S, size_t C,
                         size_t n_samples, double expl_var, int max_singular_values, size_t wiener_colsize,
                         const double *d_sos_or_null, size_t n_sections, double taper_alpha, void *d_workspace,
                         size_t workspace_bytes, bpmf_stream_t stream, float *d_filtered_or_null, float *d_stack,
                         int32_t *d_n_singular, int32_t *d_status);

/* utils.bandpass_filter (BPMF/utils.py:24-90) on every row of a (rows, n_samples) table, one thread per row: with
 * `detrend` the mean, then the least-squares line (closed form about the middle index) are subtracted; with
 * taper_alpha > 0 the row is multiplied by scipy.signal.windows.tukey(n_samples, taper_alpha) (<= 0: no taper; above
 * 1: 1); then the cascade of second-order sections runs from zero state in SciPy's operation order -- per sample,
 * sections innermost, y = b0 x + z0; z0 = (b1 x - a1 y) + z1; z1 = b2 x - a2 y -- and, with `zerophase`, once more on
 * the reversed row, reversed again.  No padding.  Without detrend and taper a float64 result equals
 * scipy.signal.sosfilt (seismic_bpmf_amd.postprocess.bandpass_filter_host) bit for bit.
 *   d_x f32 (in_f64 == 0) or f64; d_sos (n_sections, 6) f64 on the device, a0 = 1; d_out f32 or f64 (out_f64), must
 *   not overlap d_x.  Every element of the output is written.  A zero-phase call with float32 output keeps the
 *   forward pass in d_workspace: bpmf_bandpass_rows_workspace_bytes (8 rows n_samples; 0 for the other calls).
 * Returns -1 for a null pointer, n_samples == 0 or above 2^24, rows >= 2^31, 0 or more than 8 sections, a
 * taper_alpha that is NaN, or a workspace that is missing or too small.  rows == 0 launches nothing and returns 0. */
size_t bpmf_bandpass_rows_workspace_bytes(size_t rows, size_t n_samples, int zerophase, int out_f64);
int bpmf_bandpass_rows_dev(const void *d_x, int in_f64, size_t rows, size_t n_samples, const double *d_sos,
                           size_t n_sections, int detrend, double taper_alpha, int zerophase, int out_f64,
                           void *d_workspace, size_t workspace_bytes, bpmf_stream_t stream, void *d_out);

/* ------------------------------------------- multi-band displacement spectra of a day's events --- */
/*
 * Spectrum.compute_multi_band_spectrum (BPMF/spectrum.py:387-505, method "multiband" of compute_moment_magnitude) for
 * every window of a day in HBM in one call (spectrum.hip).  Windows are addressed as bpmf_normalize_batch_dev
 * addresses them: window w < n_windows = E * S starts at d_start[w] on station w % S; row (w, c), c < C, is
 *     x[i] = d_data[w % S, c, d_start[w] + i]                                                (i = 0 .. n_samples-1)
 * In float64 throughout (the definition is seismic_bpmf_amd.postprocess.multiband_spectrum_host; obspy's detrend,
 * taper and filter are restated there from their documented behaviour):
 *   1. the mean is subtracted, then the least-squares line (closed form about the middle index, as
 *      bpmf_bandpass_rows_dev), both from compensated sums;
 *   2. sample i and sample n_samples - 1 - i, i < taper, are multiplied by 0.5 (1 - cos(pi i / taper));
 *   3. for every band b with skip[b] == 0 the cascade of the n_sections sections d_sos[b] runs from zero state in
 *      SciPy's operation order, forward and then over the reversed result;
 *   4. d_out[w, c, b] = max |y[k]| over buffer <= k < n_samples - buffer, divided by bandwidths[b]; a NaN in that
 *      range gives NaN.  A band with skip[b] != 0 gives +0.
 * A window that is not wholly inside [0, N) is not processed: its outputs are +0 and d_valid[w] = 0 (1 elsewhere).
 *   d_data (S, C, N) f32; d_start (n_windows) i64 on the device, clamped to +-2^40; d_sos (n_bands, n_sections, 6) f64
 *   on the device, a0 = 1; bandwidths (n_bands) f64 and skip (n_bands) u8 ON THE HOST (read before the call returns);
 *   d_out (n_windows, C, n_bands) f64; d_valid (n_windows) u8.  Every element of both outputs is written.
 * Workspace: a row takes (4 + (1 + n_active) n_samples) * 8 bytes, n_active the bands that are not skipped; the rows
 * go through in slabs of a multiple of 64 that fit, so 64 rows' worth are the least.  A row gives the same bits in any
 * slab and any batch.  bpmf_multiband_workspace_bytes returns what n_rows = n_windows * C rows take in one slab (n_rows
 * rounded up to 64), or 0 for sizes that the call refuses.  Asynchronous on `stream`.
 * Returns -1 for a null pointer, S * C == 0, N == 0 or above 2^40, n_windows no multiple of S, n_samples == 0 or above
 * 16384, buffer == 0, n_samples <= 2 buffer, taper > n_samples / 4, n_bands outside 1 .. 64, n_sections outside 1 .. 8,
 * n_windows * C * n_bands >= 2^31, a band that is not skipped with a bandwidth that is no positive number, or a
 * workspace smaller than 64 rows.  n_windows == 0 launches nothing and returns 0.
 */
size_t bpmf_multiband_workspace_bytes(size_t n_rows, size_t n_samples, size_t n_active_bands);
int bpmf_multiband_spectrum_dev(const float *d_data, size_t S, size_t C, size_t N, size_t n_windows,
                                const int64_t *d_start, size_t n_samples, size_t taper, size_t buffer,
                                const double *d_sos, size_t n_bands, size_t n_sections, const double *bandwidths,
                                const uint8_t *skip, void *d_workspace, size_t workspace_bytes, bpmf_stream_t stream,
                                double *d_out, uint8_t *d_valid);

/* ------------------------------------------- FFT-method displacement spectra of a day's events --- */
/*
 * Spectrum.compute_spectrum and Spectrum.resample (BPMF/spectrum.py:507-599, :851-887; method "regular" of
 * compute_moment_magnitude) for every window of a day in HBM in one call (fft_spectrum.hip).  Windows are addressed as
 * bpmf_multiband_spectrum_dev addresses them; row (w, c) is x[j] = d_data[w % S, c, d_starts[w] + j], j < n_samples.
 * In float64 throughout (the definition is seismic_bpmf_amd.postprocess.fft_spectrum_host), as a DFT pruned to the
 * n_bins bins of d_bins:
 *   X[b] = delta * sum_j x[j] d_taper[j] (T[(j k) mod n][0] + i T[(j k) mod n][1]),   k = d_bins[b],
 * T = d_twiddles (n_samples, 2) = cos, -sin of 2 pi m / n_samples (postprocess.dft_twiddles); the sum runs in an order
 * that depends on n_samples only, and the product with delta is one rounded multiply each on re and im.
 *   n_targets == 0, multi_component == 0: d_out (n_windows, C, n_bins, 2) = re, im of X;
 *   n_targets == 0, multi_component != 0: d_out (n_windows, n_bins) = sqrt(sum_c |X_c|^2), summed in component order;
 *   n_targets > 0: with fp = |X| (or, multi_component, that root) d_out (n_windows, C, n_targets) or
 *     (n_windows, n_targets) holds np.interp's value: fp[p] where d_flags[t] & 1 (the target is a bin's frequency),
 *     ((fp[p + 1] - fp[p]) / d_span[t]) * d_dx[t] + fp[p] elsewhere, p = d_pair[t] an index INTO d_bins (whose next
 *     entry is the next bin), and +0 where d_flags[t] & 2 (the target is at or beyond 0.99 f_max).
 * A row that holds a NaN or an Inf gives NaN wherever it is not +0 by a flag.  A window that is not wholly inside
 * [0, N) is not processed: its outputs are +0 and d_valid[w] = 0 (1 elsewhere).
 *   d_data (S, C, N) f32; d_starts (n_windows) i64, clamped to +-2^40; d_taper (n_samples) f64; d_bins (n_bins) i32,
 *   ascending, 0 .. n_samples / 2; d_pair i32, d_dx, d_span f64, d_flags u8 (n_targets), unused (may be null) without
 *   targets; all on the device.  d_valid (n_windows) u8.  Every element of both outputs is written.
 * Workspace: a row takes 16 n_bins + 1 bytes; the rows go through in slabs of a multiple of 64 that fit, so 64 rows'
 * worth are the least.  A row gives the same bits in any slab and any batch.  bpmf_fft_spectrum_workspace_size returns
 * what n_rows = n_windows * C rows take in one slab (n_rows rounded up to 64), or 0 for sizes that the call refuses.
 * Asynchronous on `stream`.
 * Returns -1 for a null pointer, S * C == 0, N == 0 or above 2^40, n_windows no multiple of S, n_samples outside
 * 2 .. 16384, n_bins outside 1 .. n_samples / 2 + 1, n_targets above 1024, multi_component with C above 64, a delta that
 * is not finite, n_windows * C * max(2 n_bins, n_targets) >= 2^31, or a workspace smaller than 64 rows.
 * n_windows == 0 launches nothing and returns 0.
 */
size_t bpmf_fft_spectrum_workspace_size(size_t n_rows, size_t n_samples, size_t n_bins, size_t n_targets);
int bpmf_fft_spectrum_dev(const float *d_data, size_t S, size_t C, size_t N, size_t n_windows,
                          const long long *d_starts, size_t n_samples, const double *d_taper,
                          const double *d_twiddles, double delta, const int *d_bins, size_t n_bins, const int *d_pair,
                          const double *d_dx, const double *d_span, const unsigned char *d_flags, size_t n_targets,
                          int multi_component, void *d_workspace, size_t workspace_bytes, bpmf_stream_t stream,
                          double *d_out, unsigned char *d_valid);

/* --------------------- propagation corrections, network-average spectra and Mw* of a day's events --- */
/*
 * What follows the spectra in compute_moment_magnitude (BPMF/spectrum.py:1806-1880) for ONE phase of E events in one
 * call (source_spectra.hip; called by workflow.network_average_spectra and workflow.approximate_moment_magnitudes).
 * A channel is (s, c), ch = s C + c; every spectrum is (E, S * C, F) f64, as bpmf_fft_spectrum_dev and
 * bpmf_multiband_spectrum_dev leave them (C = 1 for multi_component spectra).  The stages are the bits of `flags`; the
 * definitions are seismic_bpmf_amd.postprocess.source_spectra_host and approximate_moment_magnitude_host:
 *   1 SNR         d_snr = 0 where |signal| and |noise| are both 0, where d_noise_valid[e, s] == 0 and where
 *                 d_valid[e, s] == 0; |signal| / |noise| elsewhere (compute_signal_to_noise_ratio :601-648).
 *   2 correction  d_corrected = (signal * g) * a, each product rounded, g = geometry_constant * (1000 d_dist) /
 *                 radiation, a = exp(((pi d_travel_time) d_frequencies[f]) / d_q[f]); 0 where d_valid[e, s] == 0
 *                 (correct_geometrical_spreading :200-227, correct_attenuation :229-256).
 *   4 average     compute_network_average_spectrum (:258-386) of d_corrected under d_snr: a station is used if valid
 *                 and not 100 (d_location_err[e] / d_dist[e, s]) > max_relative_distance_err_pct; per bin over the
 *                 used channels in channel order: masked where snr < snr_threshold; d_num_valid counts the unmasked;
 *                 a bin with fewer than min_num_valid is masked throughout; with average_log values <= 0, NaN and inf
 *                 are masked too and log10 is averaged, the result being exp(mean log(10)); reduce_median != 0 takes the median
 *                 (half-sum of the two middle values of an even count; NaN if an unmasked value is NaN) for the mean;
 *                 d_std = sqrt(sum((v - mean)^2) / count).  d_mask = 1 and d_average = d_std = NaN for a bin without
 *                 an unmasked channel; a mean that is not finite gives d_std = 0 and, unless the median was asked for,
 *                 d_mask = 1 and d_average = NaN, as np.ma's division masks it.
 *   8 Mw*         approximate_moment_magnitude (:1341-1496) from d_corrected and d_snr: per channel of a valid station
 *                 the value at the lowest band with snr > snr_threshold (the median of the lowest
 *                 min(k, num_averaging_bands) of k such bands) with SNR snr_threshold, or without such a band, over
 *                 the bands f >= first_high_band and with NaN terms as 0, 10 ** (sum(snr log10(v)) / sum(snr)) with SNR
 *                 sum(snr^2) / sum(snr) (a sum of 0 replaced by 1), sums in NumPy's order; the SNR is f32, 0 where
 *                 the measurement is 0.  Weights (f32): min(SNR, 1.001 snr_threshold, weight_max); 0 for SNR <
 *                 snr_threshold if at least max_num_bad_measurements are not below it, otherwise 0 for all but the
 *                 max_num_bad_measurements largest (ties by index); times the reciprocal of d_epicentral_dist clipped
 *                 to its 25th and 75th percentile (np.percentile, linear) over the S stations of the event.
 *                 d_log10_m0 = sum(log10(measurement) weight over weight > 0) / (f32 sum of weights), over the
 *                 channels of valid stations in NumPy's order; d_mw_star = scaling * (d_log10_m0 - 9.1).
 * d_corrected and d_snr are outputs of stages 2 and 1 and inputs of stages 4 and 8 when those bits are not set.
 *   d_signal, d_noise (E, S*C, F) f64; d_valid, d_noise_valid (E, S) u8; d_dist, d_epicentral_dist, d_travel_time
 *   (E, S) f64; d_location_err (E) f64; d_frequencies, d_q (F) f64; d_average, d_std (E, F) f64; d_mask (E, F) u8;
 *   d_num_valid (E, F) i32; d_used (E, S) u8; d_mw_star, d_log10_m0 (E) f64; d_measured_disp (E, S*C) f64 (NaN for a
 *   station that is not valid); d_weights, d_measurement_snr (E, S*C) f32.  All on the device; a pointer that no
 *   stage asked for reads or writes may be null.  Every element of the outputs of the stages asked for is written.
 * One wave per event, no workspace: an event gives the same bits alone and in any batch.  Asynchronous on `stream`.
 * Returns -1 for flags that are 0 or hold other bits, a null pointer that a stage needs, S * C outside 1 .. 256, F
 * outside 1 .. 1024, E * S * C * F >= 2^31, and with bit 8 num_averaging_bands outside 1 .. 8, first_high_band > F or
 * max_num_bad_measurements < 0.  E == 0 launches nothing and returns 0.
 */
int bpmf_source_spectra_dev(const double *d_signal, const double *d_noise, const unsigned char *d_valid,
                            const unsigned char *d_noise_valid, const double *d_dist,
                            const double *d_epicentral_dist, const double *d_travel_time,
                            const double *d_location_err, const double *d_frequencies, const double *d_q, size_t E,
                            size_t S, size_t C, size_t F, unsigned flags, double geometry_constant, double radiation,
                            double snr_threshold, double max_relative_distance_err_pct, int min_num_valid,
                            int average_log, int reduce_median, int num_averaging_bands, size_t first_high_band,
                            double magnitude_log_moment_scaling, double weight_max, int max_num_bad_measurements,
                            bpmf_stream_t stream, double *d_corrected, double *d_snr, double *d_average,
                            unsigned char *d_mask, double *d_std, int *d_num_valid, unsigned char *d_used,
                            double *d_mw_star, double *d_log10_m0, double *d_measured_disp, float *d_weights,
                            float *d_measurement_snr);

/* ------------------------------- Brune / Boatwright fits of the network-average spectra --- */
/*
 * Spectrum.fit_average_spectrum (BPMF/spectrum.py:729-849, log=True) with the below-fc gate and the stress drop, for ONE
 * phase of E events in one call (spectral_fit.hip; called by workflow.fit_source_spectra).  The inputs are what stage
 * 4 of bpmf_source_spectra_dev leaves.  The answer is DEFINED as the exact weighted least-squares minimum
 * (seismic_bpmf_amd.postprocess.fit_source_spectra_host), not as the point where SciPy's curve_fit stops: over the M
 * unmasked bins, y = log10(d_average), x = d_frequencies, w = 1 or, weighted, sigmoid((d_num_valid - mean) / mean) with
 * the mean over all F bins; the model is a - g(x / fc) with a = log10 Omega_0 and g = log10(1 + r^2) (model 0, Brune)
 * or 0.5 log10(1 + r^4) (model 1, Boatwright); with u = ln fc the profile cost is
 *   P(u) = 1/2 sum w^2 (y + g - a(u))^2,   a(u) = sum w^2 (y + g) / sum w^2,   sums in bin order,
 * and u* = argmin P on the closed interval [ln(fc0 / BPMF_FIT_BOUND_FACTOR), ln(fc0 * BPMF_FIT_BOUND_FACTOR)], fc0 =
 * fc_circular_crack(moment_to_magnitude(first unmasked value)) with the reference's defaults, found with fixed trip
 * counts: BPMF_FIT_SCAN_POINTS evenly spaced u, the lowest cost (ties to the lowest index, a NaN as +inf),
 * BPMF_FIT_ZOOM_ROUNDS rounds of BPMF_FIT_ZOOM_POINTS points on the bracket of the lowest point's two neighbours, then
 * BPMF_FIT_NEWTON_STEPS Newton steps u - P' / P'' (taken where P'' > 0 and the step is finite), clamped to the bracket.
 * Outputs per event: d_m0 = 10^a(u*), d_fc = exp(u*), d_mw = 2/3 (log10 M0 - 9.1), d_cost = P(u*), d_stress_drop (Pa,
 * stress_drop_circular_crack for `phase`: 0 P, 1 S), d_m0_err and d_fc_err the roots of the diagonal of
 * (2 P / (M - 2)) (J^T J)^-1 in closed form (inf for M <= 2), d_n_valid = M, d_at_bound (u* at either end), d_reason:
 *   0 fitted (d_success = 1); 1 no unmasked bin; 2 M / F < min_fraction_valid_points; 3 fewer than
 *   min_fraction_valid_points_below_fc * F unmasked bins with x < fc; 4 at a bound; 5 a y, w, M0, fc, cost, Mw or stress
 *   drop that is not finite.  The seven f64 outputs are NaN for reasons 1, 2 and 5, and reported for 3 and 4.
 *   d_average (E, F) f64; d_mask (E, F) u8; d_num_valid (E, F) i32; d_frequencies (F) f64, positive and ascending (the
 *   caller's to check); seven (E) f64, d_n_valid (E) i32, three (E) u8.  All on the device; every element is written.
 * One wave per event, no workspace: an event gives the same bits alone and in any batch.  Asynchronous on `stream`.
 * Returns -1 for a null pointer, F outside 1 .. 1024, E * F >= 2^31, a model or phase that is not 0 or 1.  E == 0
 * launches nothing and returns 0.
 */
#define BPMF_FIT_SCAN_POINTS 1024
#define BPMF_FIT_ZOOM_ROUNDS 2
#define BPMF_FIT_ZOOM_POINTS 64
#define BPMF_FIT_NEWTON_STEPS 4
#define BPMF_FIT_BOUND_FACTOR 1.0e3
int bpmf_fit_spectra_dev(const double *d_average, const unsigned char *d_mask, const int *d_num_valid,
                         const double *d_frequencies, size_t E, size_t F, int model, int phase, int weighted,
                         double min_fraction_valid_points, double min_fraction_valid_points_below_fc,
                         bpmf_stream_t stream, double *d_m0, double *d_fc, double *d_mw, double *d_m0_err,
                         double *d_fc_err, double *d_cost, double *d_stress_drop, int *d_n_valid,
                         unsigned char *d_success, unsigned char *d_at_bound, unsigned char *d_reason);

/* ------------------------------------------- events detected by several templates --- */
/*
 * The loop of TemplateGroup.remove_multiples (BPMF/dataset.py:5214-5282) on a catalog that is ALREADY in the
 * stable order of its origin times (equal times: the caller's order): unique_out[n] = 1 where event n stays
 * `unique_event`, 0 where another template's detection of the same event has the larger cc.  An event n1 that is
 * still unique gathers n1, n1+1, ... for as long as the float64 sum of the inter-event times t[k] - t[k-1],
 * accumulated left to right, stays < dt_criterion; of these, the ones still unique and with
 * pair_ok[rows[n1] * T + rows[m]] != 0 are multiples when there are two or more: all are flagged, the one with the
 * largest cc (equal cc: the earliest) is restored.  Host definition: seismic_bpmf_amd.postprocess.flag_multiples.
 *   d_t_sorted (n) f64 seconds, ascending; d_rows_sorted (n) i32 rows of pair_ok; d_cc_sorted (n) f32, finite;
 *   d_pair_ok (T, T) u8; d_unique_out (n) u8 out, every element written.
 * n == 0 returns 0 and touches nothing.  A row outside [0, T) fails the call (bpmf_last_error names the event) and
 * is never used as an index.  Synchronises `stream` once, to read that check back: on return the flags are complete.
 * A run of events without a gap of dt_criterion is walked by one wavefront (csrc/multiples.hip).
 */
size_t bpmf_flag_multiples_workspace_bytes(size_t n);
int bpmf_flag_multiples_dev(const double *d_t_sorted, const int32_t *d_rows_sorted,
                            const float *d_cc_sorted, size_t n, const uint8_t *d_pair_ok, size_t T,
                            double dt_criterion, void *d_workspace, size_t workspace_bytes,
                            bpmf_stream_t stream, uint8_t *d_unique_out);

/* ------------------------------------------------------------------- pair geometry --- */
/*
 * Source-receiver distances, utils.compute_distances (BPMF/utils.py:1419-1498) with Vincenty's inverse on WGS84
 * (|d lambda| < 1e-12, 200 iterations at most) in place of cartopy's geodesic (csrc/geometry.hip; host definition:
 * seismic_bpmf_amd.postprocess.compute_distances_host).
 *   d_sources (4, K) f64, d_receivers (4, R) f64: longitude (degrees), sin and cos of the reduced latitude
 *     atan((1 - f) tan(latitude)), depth (km).  The receiver is the geodesic's first point.
 *   d_epicentral (K, R) f32 or NULL: float32(metres / 1000).  d_metres (K, R) f64 or NULL: the geodesic's length.
 *   d_hypocentral (K, R) f32: sqrt(epicentral^2 + (depth_source - depth_receiver)^2) -- depth_float64 == 0: all in
 *     float32 (the depths must be float32 values); otherwise epicentral^2 in float32, the rest in float64, rounded
 *     to float32 at the end: NumPy's promotion when any depth is float64.
 *   d_nonconverged (1) i32: the pairs the iteration gave up on (within about 0.6 degrees of antipodal); they get
 *     pi (a + b) / 2.  Zeroed by the call.
 * No workspace, no host synchronisation; an element depends on its own pair alone.  Returns -1 for a NULL required
 * pointer or K == 0 or R == 0, before any launch.
 */
int bpmf_geo_distances_dev(const double *d_sources, size_t K, const double *d_receivers, size_t R,
                           int depth_float64, bpmf_stream_t stream, float *d_hypocentral, float *d_epicentral,
                           double *d_metres, int32_t *d_nonconverged);

/*
 * The pair matrices of a TemplateGroup (BPMF/dataset.py:4568-4688), each (T, T) f32, every element written (host
 * definition: seismic_bpmf_amd.postprocess.template_geometry_host):
 *   d_intertemplate_dist[t, u]  as bpmf_geo_distances_dev gives it for source t and receiver u, float32 depths;
 *   d_dir_errors[t, u]          float32(sqrt(3.52 |u^T C_t u|)), u = (X_u - X_t) / |X_u - X_t| (0 where u is at t), the
 *                               sums over j, then i, in index order; 15.0 for a template without covariance;
 *   d_ellipsoid_dist[t, u]      (dist[t, u] - dir_errors[t, u]) - dir_errors[u, t] in float32.
 *   d_geo (4, T) f64: longitude, sin and cos of the reduced latitude, depth (km), of the float32 coordinates.
 *   d_xyz (3, T) f64: the Cartesian coordinates of the directions (the reference: Mercator metres and depth in km).
 *   d_cov (9, T) f64 or NULL: element (i, j) of template t at [(3 i + j) T + t]; NULL: no template has one.
 *   d_has_cov (T) u8 or NULL (all have one).  d_nonconverged (1) i32 or NULL: as above.
 * Returns -1 for a NULL required pointer or T == 0, before any launch.
 */
int bpmf_template_geometry_dev(const double *d_geo, const double *d_xyz, const double *d_cov,
                               const uint8_t *d_has_cov, size_t T, bpmf_stream_t stream,
                               float *d_intertemplate_dist, float *d_dir_errors, float *d_ellipsoid_dist,
                               int32_t *d_nonconverged);

/*
 * The (T, T) u8 masks the catalogue stages read off ellipsoid_dist (T, T) f32; comparisons in float64.
 *   BPMF_PAIR_MASK_MULTIPLES      mask[i, j] = ellipsoid_dist[i, j] < criterion, and with d_intertemplate_cc
 *                                 (T, T) f32 not NULL: & (cc[i, j] >= similarity) -- postprocess.multiples_pair_mask;
 *   BPMF_PAIR_MASK_INTERTEMPLATE  mask[i, j] = !(ellipsoid_dist[j, i] > criterion): the COLUMN the reference reads
 *                                 (dataset.py:4815) -- postprocess.intertemplate_pair_mask; d_intertemplate_cc NULL.
 * A NaN fails `<` and `>`: 0 in the first mode, 1 in the second.  Returns -1 for an unknown mode, a NULL required
 * pointer or T == 0, before any launch.
 */
#define BPMF_PAIR_MASK_MULTIPLES 0
#define BPMF_PAIR_MASK_INTERTEMPLATE 1
int bpmf_pair_mask_dev(const float *d_ellipsoid_dist, const float *d_intertemplate_cc, size_t T, int mode,
                       double criterion, double similarity, bpmf_stream_t stream, uint8_t *d_mask);

/* ------------------------------------------------------------ running kurtosis --- */
/*
 * Device version of BPMF.clib.kurtosis (BPMF/clib.py:86-102 -> BPMF/libc.c:11-53): kurto[ch][n],
 * n >= W, is the kurtosis of the W samples before n; written only where the window variance
 * exceeds 1e-6 -- zero-initialise d_kurto like the reference wrapper does.
 *   d_signal, d_kurto (n_channels, length) f32, n_channels = stations x components
 * Limits: 1 <= W <= 32768 (a workgroup stages W + 256 samples in LDS: 132 096 bytes of the CU's 160 KB at the
 * largest window) and n_channels <= 65535 (gridDim.y) per call; anything beyond fails without a launch.
 * length <= W writes nothing and returns 0.
 */
int bpmf_kurtosis_dev(const float *d_signal, int W, size_t n_channels, size_t length,
                      bpmf_stream_t stream, float *d_kurto);

/* ------------------------------------------------------ peak suppression (host) --- */
/*
 * The height-ordered suppression loop of BPMF/utils.py:2334-2345 (`_detect_peaks`, mpd > 1), which
 * the reference runs as an O(peaks^2) NumPy loop: peaks are visited from the tallest down and a
 * kept peak removes every other peak within +-mpd samples.  Same visiting order (the caller passes
 * the reference's own argsort), same result, O(peaks) time.  Host arrays.
 *   positions (n) i64 ascending sample indices of the candidate peaks
 *   order     (n) i64: order[q] = index into `positions` of the q-th peak to visit
 *   keep      (n) u8 out, indexed like `positions` (1 = survives)
 */
int bpmf_suppress_peaks(const int64_t *positions, const int64_t *order, size_t n, double mpd,
                        uint8_t *keep);

/* ------------------------------------------------------------ grid decimation --- */
/*
 * Device version of BPMF.clib.find_similar_sources (BPMF/clib.py:104-221), i.e. of
 * BPMF/libc.c:find_similar_moveouts (:55-223, method 0 = "smallest") and
 * find_similar_moveouts2 (:225-387, method 1 = "closest"): the one-time O(K^2 S) decimation
 * of the source grid that precedes the backprojection.  Host arrays, same argument order as the
 * reference's C functions (num_threads replaced by the method / device); the result equals the
 * reference run single-threaded.
 *   moveouts (K, S) f32 seconds; redundant_sources (K) i32 out (1 = redundant)
 * Refused with -1 before any device work, redundant_sources untouched and the argument named in
 * bpmf_last_error(): a null pointer, K = 0, S = 0 or S > 256, n_stations_for_diff outside 1 .. S,
 * a method other than 0 / 1.
 */
int bpmf_find_similar_sources(const float *moveouts, const float *source_longitude,
                              const float *source_latitude, const float *cell_longitude,
                              const float *cell_latitude, float threshold, size_t n_sources,
                              size_t n_stations, size_t n_cells_longitude,
                              size_t n_cells_latitude, size_t n_stations_for_diff, int method,
                              int device, int32_t *redundant_sources);

#ifdef __cplusplus
}
#endif
#endif /* BPMF_HIP_H */
