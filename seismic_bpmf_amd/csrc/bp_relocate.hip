// Relocation of a BATCH of events in one backprojection call: the beamforming step of Event.relocate_beam
// (BPMF/dataset.py:2102-2269), which tutorial notebook 6 runs in a loop over every detected event.  Per event
// the reference backprojects a 60-120 s window (N ~ 1 500-3 000 samples) over the whole grid with
// reduce="none", takes np.unravel_index(beam.argmax(), beam.shape) and turns beam[:, time_idx] into a
// likelihood (BPMF/template_search.py:498-506).
//
// Events are independent and share the plan, so here they share the launches and the (K, N) volume is never
// made:
//   1. prestack   U[e, s, p, t], the fmaf chain of bp_prestack_kernel, an event's window read where it lies
//                 (its own array, or a slice of the day in HBM);
//   2. max-beam   the general beam kernels of bp.hip over gridDim.z = events (bp_max_batch): per event the
//                 running (max, arg-max) over the sources at every sample -- 8 N bytes instead of 4 K N;
//   3. focus      the global maximum M of an event's max-beam; among the samples that reach M the smallest
//                 source id, then the smallest sample.  With M > 0 that IS the first maximum of the volume in
//                 source-major order: the arg-max of a sample is the lowest source that reaches its maximum, so
//                 the lowest source that reaches M anywhere is the smallest arg among those samples, and its
//                 first such sample is the smallest of them.  (M = 0 and a volume that is not all zero -- a
//                 negative beam -- is the caller's to detect: postprocess.focus_from_max states the rule.)
//   4. column     beam[k, time_idx] of every source, one sample per source, gathered from the prestack in the
//                 oracle's order (oracle/bpmf_oracle.c:bp_cpu: stations outer, phases inner, fmaf(beta, U, b),
//                 beta == 0 skipped, out-of-range terms skipped, strict: 0 unless every used term is in range);
//   5. likelihood ((col - min) / (max - min)).clip(0, 1) in float32, one subtract and one IEEE divide per
//                 source as NumPy does them; a constant column gives 0 / 0 = NaN, which the clip keeps.
// "temporal" stops after the focus (first maximum in time) and hands the max-beam rows out.
#include "bp_plan.h"
#include <cmath>

namespace bpmf {

// ------------------------------------------------------------------- prestack ---
// Event e, station s, sample t: feat[e * event_stride + starts[e] + (s C + c) row_stride + t].  A sample outside
// its row [0, row_stride) -- which the Python caller refuses -- reads as 0 instead of leaving the array.
// MAXP > 0: one thread per (e, s, t) writes P <= MAXP phases; MAXP = 0: one thread per (e, s, p, t).
template <int MAXP>
__global__ __launch_bounds__(256) void bp_prestack_batch_kernel(const float* __restrict__ feat, size_t event_stride,
                                                                long long row_stride,
                                                                const long long* __restrict__ starts,
                                                                const float* __restrict__ w_ph, long long N, int C,
                                                                int P, float* __restrict__ U)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int s = MAXP ? blockIdx.y : blockIdx.y / P, p1 = MAXP ? 0 : blockIdx.y % P;
    const size_t e = blockIdx.z;
    if (t >= N) return;
    const long long g = (starts ? starts[e] : 0) + t;
    const bool inside = g >= 0 && g < row_stride;
    const float* __restrict__ fe = feat + e * event_stride;
    float* __restrict__ Ue = U + e * (size_t)gridDim.y * (MAXP ? (size_t)P : 1) * (size_t)N;
    constexpr int NP = MAXP ? MAXP : 1;
    float acc[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = 0.0f;
    for (int c = 0; c < C; ++c) {
        const float f = inside ? fe[((size_t)s * C + c) * (size_t)row_stride + g] : 0.0f;
#pragma unroll
        for (int p = 0; p < NP; ++p)
            if (!MAXP || p < P) acc[p] = __fmaf_rn(w_ph[((size_t)s * C + c) * P + (MAXP ? p : p1)], f, acc[p]);
    }
#pragma unroll
    for (int p = 0; p < NP; ++p)
        if (!MAXP || p < P) Ue[((size_t)s * P + (MAXP ? p : p1)) * (size_t)N + t] = acc[p];
}

// ---------------------------------------------------------------------- focus ---
struct FocusKey {
    float m;
    int arg, t;
};
// a before b: the larger maximum; spatial: then the lower source id; then the earlier sample
template <bool SPATIAL>
__device__ __forceinline__ bool focus_before(const FocusKey& a, const FocusKey& b)
{
    if (a.m != b.m) return a.m > b.m;
    if (SPATIAL && a.arg != b.arg) return a.arg < b.arg;
    return a.t < b.t;
}

// One workgroup per event over its (maxbeam, arg) row.  A NaN never compares greater: it is never the maximum,
// as in the running maximum that made the row.
template <bool SPATIAL>
__global__ __launch_bounds__(256) void bp_focus_kernel(const float* __restrict__ maxbeam, const int* __restrict__ arg,
                                                       int N, int* __restrict__ time_idx, int* __restrict__ src_idx,
                                                       float* __restrict__ max_beam)
{
    __shared__ FocusKey sh[256];
    const size_t e = blockIdx.x;
    const float* __restrict__ mb = maxbeam + e * (size_t)N;
    const int* __restrict__ ma = arg + e * (size_t)N;
    FocusKey best{-INFINITY, 0x7fffffff, 0x7fffffff};
    for (int t = threadIdx.x; t < N; t += 256) {
        const FocusKey k{mb[t], ma[t], t};
        if (focus_before<SPATIAL>(k, best)) best = k;
    }
    sh[threadIdx.x] = best;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o && focus_before<SPATIAL>(sh[threadIdx.x + o], sh[threadIdx.x]))
            sh[threadIdx.x] = sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        // (a row of nothing but NaN or -inf: sample 0, as an arg-max over no candidate)
        const bool found = sh[0].t != 0x7fffffff;
        time_idx[e] = found ? sh[0].t : 0;
        src_idx[e] = found ? sh[0].arg : ma[0];
        max_beam[e] = found ? sh[0].m : mb[0];
    }
}

// --------------------------------------------------------------------- column ---
// One thread per (event, source): the beam of source k at the event's time of maximum focusing, from the DENSE
// tables the plan was built from (moveouts (K, S, P), w_sources (K, S)) in the oracle's order.  K S P gathers per
// event from a prestack that lies in L2; neighbouring sources read neighbouring table rows.
template <int OOB>
__global__ __launch_bounds__(256) void bp_column_kernel(const float* __restrict__ U, long long N, int K, int S, int P,
                                                        const int* __restrict__ moveouts,
                                                        const float* __restrict__ w_sources,
                                                        const int* __restrict__ time_idx, float* __restrict__ column)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t e = blockIdx.y;
    if (k >= K) return;
    const float* __restrict__ Ue = U + e * (size_t)S * (size_t)P * (size_t)N;
    const long long t = time_idx[e];
    const float* __restrict__ beta = w_sources + (size_t)k * S;
    const int* __restrict__ tau = moveouts + (size_t)k * S * P;
    bool active = false, all_inside = true;
    float b = 0.0f;
    for (int s = 0; s < S; ++s) {
        const float w = beta[s];
        if (w == 0.0f) continue;
        active = true;
        for (int p = 0; p < P; ++p) {
            const long long x = t + tau[s * P + p];
            if (x < 0 || x >= N) { all_inside = false; continue; }
            b = __fmaf_rn(w, Ue[((size_t)s * P + p) * (size_t)N + (size_t)x], b);
        }
    }
    const bool computed = active && (OOB == BPMF_BP_FLEXIBLE || all_inside);
    column[e * (size_t)K + k] = computed ? b : 0.0f;
}

// ----------------------------------------------------------------- likelihood ---
// One workgroup per event: min and max of its column (a NaN in the column makes both NaN, as np.min / np.max),
// then the rescaled, clipped column.  `like` may be the column itself (every element is read and written by the
// same thread).
__global__ __launch_bounds__(1024) void bp_likelihood_kernel(const float* __restrict__ column, int K,
                                                             float* __restrict__ like)
{
    __shared__ float s_lo[16], s_hi[16];
    __shared__ int s_nan[16];
    const size_t e = blockIdx.x;
    const float* col = column + e * (size_t)K;
    float* out = like + e * (size_t)K;
    float lo = INFINITY, hi = -INFINITY;
    bool saw_nan = false;
    for (int k = threadIdx.x; k < K; k += 1024) {
        const float v = col[k];
        saw_nan |= v != v;
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o));
        hi = fmaxf(hi, __shfl_xor(hi, o));
    }
    const bool wave_nan = __ballot(saw_nan) != 0ull;
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_lo[wave] = lo; s_hi[wave] = hi; s_nan[wave] = wave_nan; }
    __syncthreads();
    bool any_nan = false;
    for (int w = 0; w < 16; ++w) {
        lo = fminf(lo, s_lo[w]);
        hi = fmaxf(hi, s_hi[w]);
        any_nan |= s_nan[w] != 0;
    }
    if (any_nan) lo = hi = __builtin_nanf("");
    const float range = __fsub_rn(hi, lo);
    for (int k = threadIdx.x; k < K; k += 1024) {
        const float v = __fdiv_rn(__fsub_rn(col[k], lo), range);
        out[k] = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);      // (not fminf / fmaxf: the clip keeps a NaN)
    }
}

namespace {
struct RelocateLayout {
    BpSchedule sch;         // prestacks and partial rows of the max-beams (bp_max_batch)
    void* sch_ws;           // the schedule's block: the prestacks U lie at its start
    float* beam;            // [E, N] the spatial method's max-beams and their sources
    int32_t* arg;
    size_t total;
};
RelocateLayout relocate_layout(void* ws, const bpmf_bp_plan* pl, size_t E, size_t N, int forced_split)
{
    RelocateLayout l;
    Carver c(ws);
    l.sch = bp_schedule(pl->shape, N, BPMF_BP_REDUCE_MAX, forced_split, E);
    l.sch_ws = c.nest(l.sch.total);
    l.beam = c.take<float>(E * N);
    l.arg = c.take<int32_t>(E * N);
    l.total = c.bytes();
    return l;
}
}  // namespace

}  // namespace bpmf

using namespace bpmf;

extern "C" size_t bpmf_bp_relocate_workspace_bytes(const bpmf_bp_plan* pl, size_t E, size_t N, size_t C)
{
    (void)C;
    if (!pl || E == 0 || N == 0) return 0;
    return relocate_layout(nullptr, pl, E, N, (int)option(OPT_BP_SPLIT)).total;
}

extern "C" int bpmf_bp_relocate_batch_dev(const bpmf_bp_plan* pl, const float* d_features, size_t event_stride,
                                          size_t row_stride, const int64_t* d_starts, const float* d_w_phases,
                                          const int32_t* d_moveouts, const float* d_w_sources, size_t E, size_t N,
                                          size_t C, int out_of_bounds, int method, void* d_workspace,
                                          size_t workspace_bytes, bpmf_stream_t stream_, int32_t* d_time_idx,
                                          int32_t* d_src_idx, float* d_max_beam, float* d_likelihood,
                                          float* d_columns, float* d_maxbeam, int32_t* d_maxbeam_sources)
{
    hipStream_t stream = (hipStream_t)stream_;
    const bool spatial = method == BPMF_BP_RELOCATE_SPATIAL;
    if (!pl || !d_features || !d_w_phases || !d_workspace || !d_time_idx || !d_src_idx || !d_max_beam ||
        (spatial ? (!d_likelihood || !d_moveouts || !d_w_sources) : (!d_maxbeam || !d_maxbeam_sources))) {
        set_error("bpmf_bp_relocate_batch_dev: null pointer");
        return -1;
    }
    if ((method != BPMF_BP_RELOCATE_SPATIAL && method != BPMF_BP_RELOCATE_TEMPORAL) ||
        (out_of_bounds != BPMF_BP_STRICT && out_of_bounds != BPMF_BP_FLEXIBLE)) {
        set_error("bpmf_bp_relocate_batch_dev: unknown out_of_bounds/method code");
        return -1;
    }
    if (E == 0) return 0;
    if (N == 0 || C == 0 || N > 0x7fffffffull || C > 0x7fffffffull || E > 65535 || row_stride < N ||
        row_stride > 0x7fffffffffffull || pl->shape.S * pl->shape.P > 65535) {
        set_error("bpmf_bp_relocate_batch_dev: bad argument (E=%zu N=%zu C=%zu row_stride=%zu; at most 65535 events "
                  "per call)", E, N, C, row_stride);
        return -1;
    }
    // the alternative conventions are conventions of the running maximum and of the strict range; the focus rule
    // and the column kernel are written for the build's own
    if (option(OPT_BP_COMPAT_FIRST_COMPUTED) != 0 || option(OPT_BP_COMPAT_STRICT_UPPER_ONLY) != 0 ||
        option(OPT_BP_COMPAT_RANGE_ALL_STATIONS) != 0) {
        set_error("bpmf_bp_relocate_batch_dev: not available under a bp.compat_* option (relocate the events one by "
                  "one with bpmf_bp_run_dev)");
        return -1;
    }
    const int forced_split = (int)option(OPT_BP_SPLIT);        // read once: the size check and the launches agree
    const RelocateLayout l = relocate_layout(d_workspace, pl, E, N, forced_split);
    if (workspace_bytes < l.total) {
        set_error("bpmf_bp_relocate_batch_dev: workspace too small (%zu < %zu)", workspace_bytes, l.total);
        return -1;
    }
    const int S = (int)pl->shape.S, P = (int)pl->shape.P, K = (int)pl->shape.K;
    float* U = (float*)l.sch_ws;
    float* beam = spatial ? l.beam : d_maxbeam;
    int32_t* arg = spatial ? l.arg : d_maxbeam_sources;
    float* column = d_columns ? d_columns : d_likelihood;
    // option debug.poison_output (tests): what no kernel writes comes back as NaN / -1
    if (option(OPT_DEBUG_POISON_OUTPUT) != 0) {
        BPMF_HIP_CHECK(hipMemsetAsync(d_time_idx, 0xFF, E * sizeof(int32_t), stream));
        BPMF_HIP_CHECK(hipMemsetAsync(d_src_idx, 0xFF, E * sizeof(int32_t), stream));
        BPMF_HIP_CHECK(hipMemsetAsync(d_max_beam, 0xFF, E * sizeof(float), stream));
        BPMF_HIP_CHECK(hipMemsetAsync(beam, 0xFF, E * N * sizeof(float), stream));
        BPMF_HIP_CHECK(hipMemsetAsync(arg, 0xFF, E * N * sizeof(int32_t), stream));
        if (spatial) {
            BPMF_HIP_CHECK(hipMemsetAsync(d_likelihood, 0xFF, E * (size_t)K * sizeof(float), stream));
            if (d_columns) BPMF_HIP_CHECK(hipMemsetAsync(d_columns, 0xFF, E * (size_t)K * sizeof(float), stream));
        }
    }
    const unsigned nb = (unsigned)((N + 255) / 256);
    if (P <= 4)
        bp_prestack_batch_kernel<4><<<dim3(nb, (unsigned)S, (unsigned)E), dim3(256), 0, stream>>>(
            d_features, event_stride, (long long)row_stride, (const long long*)d_starts, d_w_phases, (long long)N,
            (int)C, P, U);
    else
        bp_prestack_batch_kernel<0><<<dim3(nb, (unsigned)(S * P), (unsigned)E), dim3(256), 0, stream>>>(
            d_features, event_stride, (long long)row_stride, (const long long*)d_starts, d_w_phases, (long long)N,
            (int)C, P, U);
    BPMF_LAUNCH_CHECK();
    if (int rc = bp_max_batch(pl, l.sch, l.sch_ws, N, E, out_of_bounds, stream, beam, arg))
        return rc;
    if (spatial)
        bp_focus_kernel<true><<<dim3((unsigned)E), dim3(256), 0, stream>>>(beam, arg, (int)N, d_time_idx, d_src_idx, d_max_beam);
    else
        bp_focus_kernel<false><<<dim3((unsigned)E), dim3(256), 0, stream>>>(beam, arg, (int)N, d_time_idx, d_src_idx, d_max_beam);
    BPMF_LAUNCH_CHECK();
    if (!spatial) return 0;
    const dim3 cgrid((unsigned)((K + 255) / 256), (unsigned)E);
    if (out_of_bounds == BPMF_BP_STRICT)
        bp_column_kernel<BPMF_BP_STRICT><<<cgrid, dim3(256), 0, stream>>>(U, (long long)N, K, S, P, d_moveouts,
                                                                           d_w_sources, d_time_idx, column);
    else
        bp_column_kernel<BPMF_BP_FLEXIBLE><<<cgrid, dim3(256), 0, stream>>>(U, (long long)N, K, S, P, d_moveouts,
                                                                             d_w_sources, d_time_idx, column);
    BPMF_LAUNCH_CHECK();
    bp_likelihood_kernel<<<dim3((unsigned)E), dim3(1024), 0, stream>>>(column, K, d_likelihood);
    BPMF_LAUNCH_CHECK();
    return 0;
}
