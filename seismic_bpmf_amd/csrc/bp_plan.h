// Shared between bp_plan.hip (host-only planner and run schedule), bp.hip (generic beam kernels, upload, C ABI)
// and bp_fast.hip (the interior-tile production kernel): device-side plan records, the host-side result of
// planning, the schedule of a run and the plan object.
#pragma once
#include "common.h"
#include "../../include/bpmf_hip.h"

#include <mutex>
#include <vector>

namespace bpmf {

constexpr int BP_THREADS = 256;
constexpr size_t BP_LDS_MAX = 160 * 1024;

struct BpGroup {  // one LDS residency: a run of sources and the staging work they need
    int first_src, n_src, first_chunk, n_chunk;
};
struct BpChunk {  // <= BP_THREADS consecutive floats of one prestacked (station, phase) row
    int row;   // row of U (s * P + p)
    int gofs;  // first sample, relative to the tile start t0 (window moveout origin + x0)
    int dst;   // LDS float offset
    int n;     // floats in this chunk
};
struct BpSource {
    int id, tmin, tmax, nterm;  // global id, extreme used moveouts, terms padded to the chunk (0 = unused)
};

// ---- interior-tile fast path (bp_fast.hip) ----
// A group's sources are listed once more, partitioned into RUNS of equal (padded) station count,
// ascending id inside a run.  A source is `nparts` PARTS of `tp` stations (tp even, <= 16, <= 24 at
// tile 128; one part up to 16 stations); one record of `rec_dw` dwords per part:
//   uniform weights : [id, weight, addrP_0, addrS_0, addrP_1, addrS_1, ...]   LDS byte addresses
//   per-station     : [id, 0, offs_0, w_0, offs_1, w_1, ...]   offs = float offsets P | S << 16
// Padding stations address the zero slab (offset 0) with the source's weight (or weight 0).
// Records of a run are laid out so that a wave's consecutive parts are 16 records apart:
// record (first_rec + ((m / 16) * nparts + part) * 16 + m % 16) for the m-th source of the run.
struct BpRun { int first_rec, n_src, tp, nparts; };
struct BpFastGroup { int first_run, n_run, first_win, n_win; };
// Two-residency groups (sources with 33-64 stations at tile 256, see bp_fast.hip): flags in n_run
constexpr int BPF_GROUP_LOAD = 1 << 16, BPF_GROUP_STORE = 1 << 17;
constexpr int BPF_HALVES_SLOTS = 9;      // sources per wave of a multi-residency group (16 waves: 144 per group)
// one staged window of the fast path: `len` floats of row `row` starting at t0 + gofs -> LDS float
// offset dst (len a multiple of 4, dst a multiple of 4: the LDS-DMA copies move 16 bytes per lane)
struct BpWindow { int row, gofs, dst, len; };
// LDS floats [0, BPF_ZERO_SLAB) are the zero slab (padding terms read it), floats
// [BPF_DESC_OFS, BPF_DESC_OFS + 4 * BPF_DESC_MAX) hold the NEXT group's window descriptors
// (copied there while the current group is computed)
constexpr int BPF_ZERO_SLAB = 512, BPF_DESC_OFS = 512, BPF_DESC_MAX = 256;

// One station-count class of sources with its own tile (device tables of bp_fast.hip)
struct BpFastClass {
    int tile = 512;              // 512 / 256 / 128 time samples per workgroup
    bool uniform = false;        // every source's non-zero weights are equal: ready-made addresses
    bool halves = false;         // groups of <= 144 sources computed in 2-4 LDS residencies (<= 20 stations each)
    int n_pass = 1;              // halves: consecutive entries of d_groups per group of sources
    int rec_dw = 0;              // dwords per record
    int n_groups = 0;
    int desc_waves = 1;          // waves that copy the next group's window descriptors
    size_t lds_bytes = 0;
    size_t n_sources = 0;
    int max_stations = 0;        // diagnostics
    BpFastGroup* d_groups = nullptr;
    BpRun* d_runs = nullptr;
    BpWindow* d_wins = nullptr;
    int* d_recs = nullptr;
};
constexpr int BPF_MAX_CLASSES = 3;

// one entry of the per-term table of bp_beam_wps_kernel (bp.hip)
struct BpTermV {
    int off_bytes;  // LDS byte offset of the term's window origin (+ moveout)
    float beta;     // source weight of the term's station
};

constexpr int BPD_TILE = 1024;     // samples per workgroup of bp_direct.hip

// ---- what bp_plan_host decides (bp_plan.hip: no HIP call, no device) ----
// The scalar part of a plan: everything the schedule of a run (bp_schedule) and the diagnostics read.
struct BpClassShape {
    int tile = 0;                // 512 / 256 / 128 time samples per workgroup
    bool halves = false;         // groups computed in 2-4 LDS residencies
    int n_pass = 1;              // halves: consecutive group entries per group of sources
    int n_groups = 0;            // group entries
    size_t lds_bytes = 0;
    size_t n_sources = 0;
    int max_stations = 0;
};
// why a grid has no LDS plan (in this order of precedence)
enum BpDirectReason { BP_LDS_PLAN = 0, BP_DIRECT_WINDOWS = 1 /* one source's windows exceed the LDS */,
                      BP_DIRECT_TERMS = 2 /* > 256 terms per source */, BP_DIRECT_OPTION = 3 /* bp.direct */,
                      BP_DIRECT_UPPER_ONLY = 4 /* bp.compat_strict_upper_only and a negative used moveout */ };
struct BpPlanShape {
    size_t K = 0, S = 0, P = 0;
    int tpt = 2;           // time samples per thread -> tile = BP_THREADS * tpt
    int NT = 4;            // padded number of (station, phase) terms per source
    int nsv = 0;           // > 0: packed per-station records (P == 2), NSV stations padded
    int ntv = 0;           // > 0: per-term table of NTV padded terms (tile 512 without packed records)
    bool dual = false;     // dual (shifted) windows: every term offset is even
    int n_groups = 0;
    size_t lds_bytes = 0;  // largest group
    // no LDS plan exists for this grid: bp_direct.hip gathers from global memory along compact per-source term lists
    bool direct = false;
    int direct_reason = BP_LDS_PLAN;
    // interior-tile fast path: 1-3 station-count classes of sources, each with its own tile
    bool fast = false;
    bool fast_shares_generic = false;  // the single class was built from the generic (dual) plan: the
                                       // edge tiles run the 8-byte-gather flavour of the generic kernel
    int n_classes = 0;
    BpClassShape cls[BPF_MAX_CLASSES];
    int tmin_all = 0, tmax_all = 0;    // extreme used moveouts over all sources
    int id_offset = 0;
};

struct PlanHost {               // the LDS plan of the general kernels, or of one station-count class
    std::vector<BpGroup> groups;
    std::vector<BpChunk> chunks;
    std::vector<BpSource> srcs;   // in processing order
    std::vector<int> off;
    std::vector<float> beta;
    size_t lds_floats = 0;
    int NT = 4;
    int n_pass = 1;             // > 1: every group is n_pass consecutive entries of `groups` (LDS residencies)
    int per = 0;                // n_pass > 1: weighted stations of a source per residency
    int slots = 0;              // n_pass > 1: sources per wave of a group (6, or 9 when every weight is uniform)
};
// interior-tile fast path: host-side tables of one station-count class (bp_fast.hip)
struct FastHost {
    std::vector<BpFastGroup> fg;
    std::vector<BpRun> fr;
    std::vector<BpWindow> fw;
    std::vector<int> rec;
    bool uniform = true;
    int rec_dw = 0, max_sta = 0;
    size_t n_sources = 0;
};
struct ClassHost {
    PlanHost ph;
    FastHost fh;
    int tile = 0;
    bool halves = false;
};
// Everything decided for one moveout table: the shape and the host tables that bp_plan_upload (bp.hip) copies
// to the device as they are.
struct BpPlanHost {
    BpPlanShape shape;
    std::vector<ClassHost> classes;     // the classes built (uploaded when shape.fast)
    PlanHost own;                       // the general kernels' own single-window plan ...
    bool general_is_class0 = false;     // ... unless class 0 doubles as their plan (dual windows)
    const PlanHost& general() const { return general_is_class0 ? classes[0].ph : own; }
    std::vector<int4> recs, hdr2;       // shape.nsv: packed per-station records [K, nsv/2], headers [K]
    std::vector<BpTermV> termsv;        // shape.ntv: [K, ntv]
    // shape.direct: {any station used, tmin, tmax, -} [K], first term of every source [K + 1],
    // {row, moveout, weight bits, -}: stations ascending, phases inside
    std::vector<int4> dhdr;
    std::vector<long long> dfirst;
    std::vector<int4> dterms;
};
// null, or why these arguments make no plan
const char* bp_plan_refusal(const int32_t* moveouts, const float* w_sources, size_t K, size_t S, size_t P);
BpPlanHost bp_plan_host(const int32_t* moveouts, const float* w_sources, size_t K, size_t S, size_t P,
                        int32_t source_id_offset);

// ---- the schedule of one run: which path, which kernel, how many partial rows and where they lie ----
enum BpPath { BP_PATH_DIRECT = 0, BP_PATH_INTERIOR = 1 /* interior classes + edge tiles */, BP_PATH_GENERAL = 2 };
enum BpFamily { BP_FAMILY_NONE = 0 /* direct plan */, BP_FAMILY_WPS2 = 1, BP_FAMILY_WPS = 2, BP_FAMILY_READLANE = 3 };
// the general kernel of a plan (dispatch_beam of bp.hip instantiates exactly these)
struct BpKernel {
    int family = BP_FAMILY_NONE;
    int wpb = 0, nsv = 0, b64 = 0;      // wps2: waves per workgroup, padded stations, 8-byte gathers
    int ntv = 0;                        // wps: padded terms
    int tpt = 0, nblk = 0;              // readlane: samples per thread, blocks of 64 terms
    int tile = 0;                       // samples per workgroup
    size_t lds_bytes = 0;               // dynamic LDS of the launch
    int waves_per_cu = 0, gather_bytes = 0;
};
struct BpSchedule {
    int path = BP_PATH_GENERAL;
    BpKernel kernel;
    int n_split = 1;                    // group (direct: source) ranges per tile; interior: of every class kernel
    int n_split_edge = 1;               // ... of the general kernel on the samples outside [lo_s, hi_s)
    int rows = 1;                       // partial (beam, arg) rows per series that the launches write; > 1: merged
    long long lo_s = 0, hi_s = 0;       // BP_PATH_INTERIOR: the samples of the class kernels (else empty)
    // byte offsets in the workspace: prestack(s), partial beam rows, partial arg rows; bytes of all of it
    size_t o_prestack = 0, o_pbeam = 0, o_parg = 0, total = 0;
};
BpKernel bp_general_kernel(const BpPlanShape& sh);
// `forced_split` = option bp.split as the CALLER read it (once per call: the size check of the workspace and the
// launches must see the same value even if another thread sets the option in between).
// `n_events` = 0: one series as bpmf_bp_run_dev runs it; E >= 1: a batch of E series of reduce="max" as
// bp_max_batch runs it (always the general or the direct kernel over every tile, partial rows per event).
BpSchedule bp_schedule(const BpPlanShape& sh, size_t N, int reduce, int forced_split, size_t n_events);
// source ranges per tile of reduce="max" on a plan without LDS windows
int direct_split_count(const BpPlanShape& sh, size_t N);

}  // namespace bpmf

struct bpmf_bp_plan {
    int device = 0;
    bpmf::BpPlanShape shape;
    bpmf::BpGroup* d_groups = nullptr;
    bpmf::BpChunk* d_chunks = nullptr;
    bpmf::BpSource* d_srcs = nullptr;
    int* d_off = nullptr;
    float* d_beta = nullptr;
    int4* d_recs = nullptr;      // shape.nsv: [K, nsv/2]
    int4* d_hdr2 = nullptr;      // [K] headers with the station count in .w
    bpmf::BpTermV* d_termsv = nullptr;    // shape.ntv: [K, ntv]
    bpmf::BpFastClass cls[bpmf::BPF_MAX_CLASSES];      // shape.fast: the device tables of shape.cls
    int4* d_dhdr = nullptr;            // shape.direct: BpPlanHost::dhdr, dfirst, dterms
    long long* d_dfirst = nullptr;
    int4* d_dterms = nullptr;
    // the few edge tiles of a day run the general kernel on a side stream, beside the interior
    // kernel (fork / join through the two events): a serial launch of 3-6 workgroups would add the
    // full duration of one tile (5 ms at cfg3) to every call.  A plan serves one call at a time.
    // The stream belongs to the device (context.h: one per device and process, shared by its plans, never
    // destroyed); the events are the plan's own.
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // Two host threads may run the same resident plan on different streams: the fork / join
    // sequence on the shared side stream is enqueued under this mutex, so that the sequences of
    // two calls never interleave (each call's edge tiles stay ordered behind ITS prestack kernel).
    mutable std::mutex enqueue_mutex;
};

namespace bpmf {
// bp.hip: reduce="max" of a batch of E short series (bp_relocate.hip) under sch = bp_schedule(shape, N, max, bp.split,
// E): prestacks S P N floats apart from d_workspace on, the partial rows of the split where sch says, results N
// elements apart in beam / arg
int bp_max_batch(const bpmf_bp_plan* pl, const BpSchedule& sch, void* d_workspace, size_t N, size_t E,
                 int out_of_bounds, hipStream_t stream, float* beam, int32_t* arg);
// bp_fast.hip: running (max, arg-max) over the sources of one class for its tiles [tile_lo, tile_hi)
// (units of fc.tile samples), every one of which lies inside [-tmin_all, N - tmax_all) (no bounds
// test per source).
int launch_beam_fast(const BpFastClass& fc, int id_offset, const float* U, size_t N, long long tile_lo,
                     long long tile_hi, hipStream_t stream, float* beam, int32_t* arg,
                     int n_split = 1, long long split_stride = 0, float best0 = 0.0f);
// bp_direct.hip: the whole series for a plan without LDS windows (pl->direct)
int launch_beam_direct(const bpmf_bp_plan* pl, const float* U, size_t N, int oob, int reduce,
                       hipStream_t stream, float* beam, int32_t* arg, int n_split, long long split_stride,
                       float best0);
}
