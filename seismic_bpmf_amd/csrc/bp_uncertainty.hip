// Location uncertainties of a BATCH of relocated events: the end of Event.relocate_beam (BPMF/dataset.py:
// 2207-2245) behind the beamforming of bp_relocate.hip, on the events' rows where they lie in HBM.  Per event the
// reference cuts a rectangular domain around the new epicentre (Beamformer._rectangular_domain,
// BPMF/template_search.py:1232-1267), takes the likelihood of the sources inside it and turns them into
//   hunc = sum w d / sum w     d: length in km of the WGS84 geodesic from the epicentre to the source
//   vunc = sum w |z0 - z| / sum w
// (Beamformer._compute_location_uncertainty, :1269-1333).
//
// An event is a stream of TERMS (source row r, weight w float32 widened to float64, flag "takes part"):
//   spatial   the K sources; w = likelihood[e, k]; flag = the domain test, the float64 subtract / abs / multiply /
//             compare NumPy performs (postprocess.rectangular_domain), contraction off: the same booleans;
//   temporal  the N samples; r = maxbeam_sources[e, t] - id_offset; w = expf(-(M_e - maxbeam[e, t]) / kT) in float32
//             (subtract, negate, IEEE divide, expf: NumPy's steps); flag = w > gibbs_cutoff.
// The geodesic length is Vincenty's inverse as postprocess.geodesic_distance_m states it, operation for operation:
// |d lambda| < 1e-12, at most 200 iterations, pi (a + b) / 2 for a pair that does not converge; a lane that has
// converged stops iterating and its length comes from one evaluation at its final lambda.
//
// The weights are float32, and so is the reference's DENOMINATOR: np.sum(likelihood) of a float32 vector is a
// float32 sum in NumPy's order (chunks of 8192, each summed pairwise), about 1e-7 from the exact sum.  The
// numerators np.sum(likelihood * d) are float64.  To give the reference's numbers the denominator here is that
// float32 sum, bit for bit (np_order.h and the final kernel below); the numerators are float64 sums.
//
// Four launches per call, all on the caller's stream:
//   count    grid (terms / 256, events): the flag of every term, per workgroup the number that take part (and the
//            domain mask);
//   scan     one workgroup per event: where each workgroup's terms start among the event's;
//   terms    the same grid: the flag again (cheap), the weight written to its place in the event's compacted
//            vector -- what NumPy's boolean index makes -- the geodesic length, and per workgroup the float64 sums
//            of w d and w |dz| by a fixed tree in LDS;
//   final    one workgroup per event: the workgroups' sums (strided rows, then the same tree), the float32
//            denominator, the outputs.
// One term per thread: a batch of 64 events at K = 50 000 is 12 544 workgroups and one of 2 500 is 490 000 -- the
// chip is full either way.  The event's scalars (row, epicentre, table values at its row) have a
// workgroup-uniform address: they load once per wave into scalar registers.  Lanes diverge in the iteration only
// by its trip count (4-5 on a regional grid; the wave runs the longest of its lanes) and by the flag: a
// workgroup none of whose terms takes part skips the geodesic altogether.  No floating-point atomics: the sums of
// an event depend on its own terms alone, not on the batch, the chunk or the run.
#include "bp_plan.h"
#include "geodesic.h"
#include "np_order.h"
#include <cmath>

namespace bpmf {
namespace {

constexpr int UNC_THREADS = 256;

// The fixed tree over the 256 threads of a workgroup: every thread returns with the sums.
__device__ __forceinline__ void unc_tree(double& s0, double& s1)
{
    __shared__ double sh[2][UNC_THREADS];
    const int tid = threadIdx.x;
    sh[0][tid] = s0;
    sh[1][tid] = s1;
    __syncthreads();
    for (int h = UNC_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) {
            sh[0][tid] += sh[0][tid + h];
            sh[1][tid] += sh[1][tid + h];
        }
        __syncthreads();
    }
    s0 = sh[0][0];
    s1 = sh[1][0];
}

struct UncTables {
    const double* __restrict__ tab;      // (6, K): longitude, latitude, depth, dist_per_lat, sin u, cos u
    int K, id_offset;
};

// Term i of event e: its source row, its float32 weight, whether it takes part.  r0c: the event's row.
template <bool SPATIAL>
__device__ __forceinline__ bool unc_term(const UncTables& T, size_t e, int i, int n_terms, int r0c,
                                         const float* __restrict__ values, const int32_t* __restrict__ term_src,
                                         const float* __restrict__ max_beam, double dist_per_lon, double half_side,
                                         float kT, float cutoff, int& r, float& wf)
{
#pragma clang fp contract(off)
    const size_t K = (size_t)T.K;
    if (SPATIAL) {
        r = i;
        wf = values[e * K + i];
        const double dx = fabs(T.tab[r] - T.tab[r0c]) * dist_per_lon;
        const double dy = fabs(T.tab[K + r] - T.tab[K + r0c]) * T.tab[3 * K + r0c];
        return (dx < half_side) & (dy < half_side);
    }
    r = term_src[e * (size_t)n_terms + i] - T.id_offset;
    const float x = max_beam[e] - values[e * (size_t)n_terms + i];
    wf = expf(__fdiv_rn(-x, kT));
    return wf > cutoff;
}

// number of the workgroup's threads below this one whose flag is set, and (total) of all of them
__device__ __forceinline__ int unc_rank(bool in, int& total)
{
    __shared__ int wave_n[UNC_THREADS / 64];
    const unsigned long long m = __ballot(in);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_n[wave] = __popcll(m);
    __syncthreads();
    int before = __popcll(m & ((1ull << lane) - 1ull));
    total = 0;
    for (int w = 0; w < UNC_THREADS / 64; ++w) {
        if (w < wave) before += wave_n[w];
        total += wave_n[w];
    }
    return before;
}

// 1. count: cnt[e, block] = terms of the block that take part; the (E, K) domain mask if asked for
template <bool SPATIAL>
__global__ __launch_bounds__(UNC_THREADS) void bp_unc_count_kernel(
    const int32_t* __restrict__ src_idx, UncTables T, int n_terms, const float* __restrict__ values,
    const int32_t* __restrict__ term_src, const float* __restrict__ max_beam, double dist_per_lon, double half_side,
    float kT, float cutoff, int* __restrict__ cnt, unsigned char* __restrict__ mask)
{
    const size_t e = blockIdx.y;
    const int i = blockIdx.x * UNC_THREADS + threadIdx.x;
    const int r0 = src_idx[e] - T.id_offset;
    const int r0c = (r0 >= 0 && r0 < T.K) ? r0 : 0;      // (a row outside the tables: the last stage reports it)
    bool in = false;
    if (i < n_terms) {
        int r;
        float wf;
        in = unc_term<SPATIAL>(T, e, i, n_terms, r0c, values, term_src, max_beam, dist_per_lon, half_side, kT, cutoff,
                               r, wf);
        if (SPATIAL && mask) mask[e * (size_t)T.K + i] = in ? 1 : 0;
    }
    int total;
    unc_rank(in, total);
    if (threadIdx.x == 0) cnt[e * gridDim.x + blockIdx.x] = total;
}

// 2. scan: base[e, block] = terms that take part in the blocks before it; base[e, n_blocks] = all of them
__global__ __launch_bounds__(UNC_THREADS) void bp_unc_scan_kernel(const int* __restrict__ cnt, int n_blocks,
                                                                 int* __restrict__ base)
{
    __shared__ int seg_n[UNC_THREADS];
    const size_t e = blockIdx.x;
    const int seg = (n_blocks + UNC_THREADS - 1) / UNC_THREADS;
    const int j0 = min(n_blocks, (int)threadIdx.x * seg), j1 = min(n_blocks, j0 + seg);
    int n = 0;
    for (int j = j0; j < j1; ++j) n += cnt[e * (size_t)n_blocks + j];
    seg_n[threadIdx.x] = n;
    __syncthreads();
    int run = 0;
    for (int t = 0; t < (int)threadIdx.x; ++t) run += seg_n[t];
    for (int j = j0; j < j1; ++j) {
        base[e * (size_t)(n_blocks + 1) + j] = run;
        run += cnt[e * (size_t)n_blocks + j];
    }
    if (threadIdx.x == UNC_THREADS - 1) base[e * (size_t)(n_blocks + 1) + n_blocks] = run;
}

// 3. terms: the weights that take part, compacted in term order into cw[e, 0 .. n) (what NumPy's boolean index
// makes), and per block the float64 sums of w d and w |dz| -- part (E, n_blocks, 2)
template <bool SPATIAL>
__global__ __launch_bounds__(UNC_THREADS) void bp_unc_partial_kernel(
    const int32_t* __restrict__ src_idx, UncTables T, int n_terms, const float* __restrict__ values,
    const int32_t* __restrict__ term_src, const float* __restrict__ max_beam, double dist_per_lon, double half_side,
    float kT, float cutoff, const int* __restrict__ base, float* __restrict__ cw, double* __restrict__ part)
{
#pragma clang fp contract(off)
    const size_t e = blockIdx.y;
    const int i = blockIdx.x * UNC_THREADS + threadIdx.x;
    const size_t K = (size_t)T.K;
    const int r0 = src_idx[e] - T.id_offset;
    const int r0c = (r0 >= 0 && r0 < T.K) ? r0 : 0;
    int r = 0;
    float wf = 0.0f;
    bool in = false;
    if (i < n_terms)
        in = unc_term<SPATIAL>(T, e, i, n_terms, r0c, values, term_src, max_beam, dist_per_lon, half_side, kT, cutoff,
                               r, wf);
    int total;
    const int rank = unc_rank(in, total);
    double swd = 0.0, swz = 0.0;
    if (in) {
        cw[e * (size_t)n_terms + base[e * (size_t)(gridDim.x + 1) + blockIdx.x] + rank] = wf;
        const double w = (double)wf;
        double d_km, dz;
        if (r >= 0 && r < T.K) {
            d_km = vin_length_m(T.tab[r0c], T.tab[4 * K + r0c], T.tab[5 * K + r0c], T.tab[r], T.tab[4 * K + r],
                                T.tab[5 * K + r]) / 1000.0;
            dz = fabs(T.tab[2 * K + r0c] - T.tab[2 * K + r]);
        } else {                                       // a source id that is not of this plan: not a number
            d_km = dz = __longlong_as_double(0x7ff8000000000000ll);
        }
        swd = w * d_km;
        swz = w * dz;
    }
    if (total == 0) {                                  // (uniform) nobody took part: the sums are zero
        if (threadIdx.x == 0) part[2 * (e * gridDim.x + blockIdx.x)] = part[2 * (e * gridDim.x + blockIdx.x) + 1] = 0.0;
        return;
    }
    unc_tree(swd, swz);
    if (threadIdx.x == 0) {
        const size_t o = e * gridDim.x + blockIdx.x;
        part[2 * o] = swd;
        part[2 * o + 1] = swz;
    }
}

// 4. final: one workgroup per event.  Numerators: the blocks' float64 sums, strided rows then the tree.
// Denominator: np.sum of the float32 vector cw[e, 0 .. n) in NumPy's order (np_order.h), about 1e-7 from the exact
// sum, as the reference divides by it -- two chunks per round: every leaf of a chunk holds a multiple of NP_SLOT (a
// leaf below the root has at least 64 elements), thread s finds the leaf that holds 64 s and sums it if 64 s is the
// first multiple in it; one thread per chunk then folds the leaves in order (NpFold, its values in LDS), and thread 0
// adds the chunks in order, from 0.0f.
__global__ __launch_bounds__(UNC_THREADS) void bp_unc_final_kernel(
    const int32_t* __restrict__ src_idx, UncTables T, int n_terms, int n_blocks, const double* __restrict__ part,
    const int* __restrict__ base, const float* __restrict__ cw, double* __restrict__ hunc, double* __restrict__ vunc,
    int32_t* __restrict__ n_domain, double* __restrict__ o_lon, double* __restrict__ o_lat,
    double* __restrict__ o_dep)
{
#pragma clang fp contract(off)
    constexpr int NP_SLOT = 64, PER = NP_CHUNK / NP_SLOT;   // 128 candidate leaves per chunk, 2 chunks per round
    __shared__ float leaf[2][PER];
    __shared__ float chunk_sum[2];
    __shared__ float fold_value[2][NP_MAX_DEPTH + 1];
    const size_t e = blockIdx.x;
    const int tid = threadIdx.x;
    double swd = 0.0, swz = 0.0;
    for (int j = tid; j < n_blocks; j += UNC_THREADS) {
        const size_t o = e * (size_t)n_blocks + j;
        swd += part[2 * o];
        swz += part[2 * o + 1];
    }
    unc_tree(swd, swz);
    const int n = base[e * (size_t)(n_blocks + 1) + n_blocks];
    const float* __restrict__ a = cw + e * (size_t)n_terms;
    float den = 0.0f;
    const int which = tid / PER, slot = tid % PER;
    for (int c0 = 0; c0 * NP_CHUNK < n; c0 += 2) {
        const int c = c0 + which;
        const int m = min(NP_CHUNK, n - c * NP_CHUNK);              // this chunk's length (<= 0: no such chunk)
        const int cand = slot * NP_SLOT;
        if (cand < m) {
            const NpLeaf l = np_leaf_of(m, cand);
            const float* ac = a + (size_t)c * NP_CHUNK;
            if ((l.off + NP_SLOT - 1) / NP_SLOT == slot)
                leaf[which][slot] = np_leaf_sum<float>([=](int i) { return ac[i]; }, l.off, l.len);
        }
        __syncthreads();
        if (slot == 0 && m > 0) {
            NpFold<float> fold{fold_value[which], 0};
            np_walk(m, [&](const NpLeaf& l) { fold.push(leaf[which][(l.off + NP_SLOT - 1) / NP_SLOT], l.depth); });
            chunk_sum[which] = fold_value[which][0];
        }
        __syncthreads();
        if (tid == 0) {
            den += chunk_sum[0];
            if (n - (c0 + 1) * NP_CHUNK > 0) den += chunk_sum[1];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const int r0 = src_idx[e] - T.id_offset;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (r0 < 0 || r0 >= T.K) {
        hunc[e] = vunc[e] = o_lon[e] = o_lat[e] = o_dep[e] = nan;
        n_domain[e] = -1;
        return;
    }
    const size_t K = (size_t)T.K;
    hunc[e] = swd / (double)den;                       // sum w = 0: 0 / 0, not a number, as NumPy gives
    vunc[e] = swz / (double)den;
    n_domain[e] = n;
    o_lon[e] = T.tab[r0];
    o_lat[e] = T.tab[K + r0];
    o_dep[e] = T.tab[2 * K + r0];
}

size_t unc_blocks(size_t n_terms) { return (n_terms + UNC_THREADS - 1) / UNC_THREADS; }

struct UncLayout {
    double* part;                                      // the float64 block sums
    int *cnt, *base;
    float* cw;
    size_t total;
};
UncLayout unc_layout(void* ws, size_t E, size_t n_terms)
{
    const size_t nb = unc_blocks(n_terms);
    UncLayout l;
    Carver c(ws);
    l.part = c.take<double>(E * nb * 2);
    l.cnt = c.take<int>(E * nb);
    l.base = c.take<int>(E * (nb + 1));
    l.cw = c.take<float>(E * n_terms);
    l.total = c.bytes();
    return l;
}

}  // namespace
}  // namespace bpmf

using namespace bpmf;

extern "C" size_t bpmf_bp_location_uncertainty_workspace_bytes(size_t E, size_t n_terms)
{
    if (E == 0 || n_terms == 0 || E > 65535 || n_terms > 0x7fff0000ull) return 0;     // (sizes the call refuses)
    return unc_layout(nullptr, E, n_terms).total;
}

extern "C" int bpmf_bp_location_uncertainty_dev(const bpmf_bp_plan* pl, int method, size_t E, size_t N,
                                                const int32_t* d_src_idx, const float* d_likelihood,
                                                const float* d_maxbeam, const int32_t* d_maxbeam_sources,
                                                const float* d_max_beam, const double* d_tables, double dist_per_lon,
                                                double half_side_km, double effective_kT, double gibbs_cutoff,
                                                void* d_workspace, size_t workspace_bytes, bpmf_stream_t stream_,
                                                double* d_hunc, double* d_vunc, int32_t* d_n_domain,
                                                double* d_longitude, double* d_latitude, double* d_depth,
                                                uint8_t* d_domain_mask)
{
    const char* me = "bpmf_bp_location_uncertainty_dev";
    hipStream_t stream = (hipStream_t)stream_;
    if (method != BPMF_BP_RELOCATE_SPATIAL && method != BPMF_BP_RELOCATE_TEMPORAL) {
        set_error("%s: unknown method code %d", me, method);
        return -1;
    }
    const bool spatial = method == BPMF_BP_RELOCATE_SPATIAL;
    if (!pl || !d_src_idx || !d_tables || !d_workspace || !d_hunc || !d_vunc || !d_n_domain || !d_longitude ||
        !d_latitude || !d_depth || (spatial ? !d_likelihood : (!d_maxbeam || !d_maxbeam_sources || !d_max_beam))) {
        set_error("%s: null pointer", me);
        return -1;
    }
    if (!spatial && d_domain_mask) {
        set_error("%s: the domain mask belongs to the spatial method", me);
        return -1;
    }
    if (E == 0) return 0;
    const size_t K = pl->shape.K, n_terms = spatial ? K : N;
    if (E > 65535 || K == 0 || K > 0x7fff0000ull || n_terms == 0 || n_terms > 0x7fff0000ull) {
        set_error("%s: bad argument (E=%zu K=%zu N=%zu; at most 65535 events per call)", me, E, K, N);
        return -1;
    }
    const float kT = (float)effective_kT, cutoff = (float)gibbs_cutoff;
    if (spatial ? !(half_side_km > 0.0 && std::isfinite(half_side_km) && std::isfinite(dist_per_lon))
                : !(kT > 0.0f && std::isfinite(kT) && std::isfinite(cutoff))) {
        set_error("%s: bad argument (half_side_km=%g dist_per_lon=%g effective_kT=%g gibbs_cutoff=%g)", me,
                  half_side_km, dist_per_lon, effective_kT, gibbs_cutoff);
        return -1;
    }
    const UncLayout l = unc_layout(d_workspace, E, n_terms);
    const size_t need = l.total;
    if (workspace_bytes < need) {
        set_error("%s: workspace too small (%zu < %zu)", me, workspace_bytes, need);
        return -1;
    }
    // option debug.poison_output (tests): what no kernel writes comes back as NaN / -1
    if (option(OPT_DEBUG_POISON_OUTPUT) != 0) {
        for (double* p : {d_hunc, d_vunc, d_longitude, d_latitude, d_depth})
            BPMF_HIP_CHECK(hipMemsetAsync(p, 0xFF, E * sizeof(double), stream));
        BPMF_HIP_CHECK(hipMemsetAsync(d_n_domain, 0xFF, E * sizeof(int32_t), stream));
        BPMF_HIP_CHECK(hipMemsetAsync(d_workspace, 0xFF, need, stream));
        if (d_domain_mask) BPMF_HIP_CHECK(hipMemsetAsync(d_domain_mask, 0xFF, E * K, stream));
    }
    const unsigned nb = (unsigned)unc_blocks(n_terms);
    const UncTables T{d_tables, (int)K, pl->shape.id_offset};
    const dim3 grid(nb, (unsigned)E), wg(UNC_THREADS);
    const int nt = (int)n_terms;
    if (spatial)
        bp_unc_count_kernel<true><<<grid, wg, 0, stream>>>(d_src_idx, T, nt, d_likelihood, nullptr, nullptr,
                                                           dist_per_lon, half_side_km, kT, cutoff, l.cnt, d_domain_mask);
    else
        bp_unc_count_kernel<false><<<grid, wg, 0, stream>>>(d_src_idx, T, nt, d_maxbeam, d_maxbeam_sources, d_max_beam,
                                                            dist_per_lon, half_side_km, kT, cutoff, l.cnt, nullptr);
    BPMF_LAUNCH_CHECK();
    bp_unc_scan_kernel<<<dim3((unsigned)E), wg, 0, stream>>>(l.cnt, (int)nb, l.base);
    BPMF_LAUNCH_CHECK();
    if (spatial)
        bp_unc_partial_kernel<true><<<grid, wg, 0, stream>>>(d_src_idx, T, nt, d_likelihood, nullptr, nullptr,
                                                             dist_per_lon, half_side_km, kT, cutoff, l.base, l.cw, l.part);
    else
        bp_unc_partial_kernel<false><<<grid, wg, 0, stream>>>(d_src_idx, T, nt, d_maxbeam, d_maxbeam_sources,
                                                              d_max_beam, dist_per_lon, half_side_km, kT, cutoff, l.base,
                                                              l.cw, l.part);
    BPMF_LAUNCH_CHECK();
    bp_unc_final_kernel<<<dim3((unsigned)E), wg, 0, stream>>>(d_src_idx, T, nt, (int)nb, l.part, l.base, l.cw, d_hunc,
                                                             d_vunc, d_n_domain, d_longitude, d_latitude, d_depth);
    BPMF_LAUNCH_CHECK();
    return 0;
}
