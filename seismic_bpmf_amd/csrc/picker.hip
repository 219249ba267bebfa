// What surrounds the deep-learning phase picker, on the device (BPMF/utils.py: normalize_batch :1966-2036, find_picks
// :2039-2094; the definitions are postprocess.normalize_batch_host and postprocess.find_picks_host, and the device
// equals them bit for bit).
//
// bpmf_normalize_batch_dev -- the running Z-score in front of the model.  Row (r, c) is cut by the rule of day_rows.h:
// windows of E events x S stations of the day, or, with S = rows, N = n and no starts, an already cut (R, C, n) tensor.
// One workgroup of 256 threads per row:
//   1. the row, reflect-padded by `shift` on both sides, is staged in LDS once (n + 2 shift floats);
//   2. window k covers padded[k shift, k shift + W): it is copied to a second LDS buffer (block_std squares its row in
//      place) and np.mean / np.std come from the NumPy-order float32 sums of np_sums.h.  The reference overwrites the
//      first window's statistics with the second's and the last's with the last but one's, so only windows
//      1 .. n_windows - 2 are computed (window 0 alone when there are two); std == 0 becomes 1;
//   3. every sample looks up its node interval as np.interp does -- beyond the last node: the last value; before the
//      first: the first; else a right bisection, the value itself at a node and at the last node -- interpolates mean
//      and std in float64 as slope * (t - node[j]) + value[j], every operation rounded on its own, and stores
//      ((double) x - mean) / std as float64 or as its (float).  The nodes are np.linspace's, computed on the host.
//      np.interp's second attempt behind a NaN result only matters for infinite samples, which are out of scope.
// LDS: 4 (n + 2 shift + W + 2 n_windows) bytes, at most PK_NORM_LDS_BYTES: n = 16384 with W = 3000 needs 90 KB.
//
// bpmf_find_picks_dev -- scipy.signal.find_peaks(height=thr, prominence=0.9 thr, width=1) and the moments of
// find_picks behind the model.  One workgroup per probability series, staged in LDS (n <= 16384):
//   1. every thread scans a contiguous stretch for rising edges x[i-1] < x[i], follows the plateau and keeps its
//      midpoint if a fall ends it and x >= thr (float32 -> float64 is exact and monotonic: the comparisons among
//      samples are made in float32, those with the threshold in float64).  A block scan of the counts makes the
//      candidate list ascending;
//   2. one lane per candidate walks out for the prominence (lowest sample on either side before a higher one) and in
//      for the width at half prominence (interpolated crossings); a candidate below the floor or narrower than 1 goes;
//   3. a second scan ranks the survivors; one lane per survivor of rank < max_picks sums samples * prob (float64),
//      prob (float32) and (samples - mean)^2 (float64) over int(left_ip) .. int(right_ip) as np.sum does (np_order.h:
//      np_sum, in one thread) and writes its record.  count is the true number of picks.
// Plain vector stores, no atomics; every output element is written.
#include "common.h"
#include "day_rows.h"
#include "np_sums.h"
#include <cmath>
#include "../../include/bpmf_hip.h"

namespace bpmf {

constexpr int PK_THREADS = TP_THREADS;
constexpr size_t PK_NORM_LDS_BYTES = 150 * 1024;       // dynamic; the static SumScratch takes 5 KB of the 160 KB
constexpr int PK_MAX_SERIES = 16384;                   // find_picks: 4 (n + n/2 + 1) bytes of LDS
constexpr int PK_MAX_PICKS = 4096;

template <typename OutT>
__global__ __launch_bounds__(PK_THREADS) void normalize_batch_kernel(
    const float* __restrict__ data, int S, int C, long long N, const long long* __restrict__ start, int n, int W,
    int shift, int nw, const double* __restrict__ nodes, const LeafTable tab, OutT* __restrict__ out)
{
    extern __shared__ __align__(16) float pk_lds[];
    __shared__ SumScratch scratch;
    const int n_pad = n + 2 * shift;
    float* row = pk_lds;                                           // the reflect-padded row
    float* win = row + n_pad;                                      // one window, squared in place by block_std
    float* w_mean = win + W;
    float* w_std = w_mean + nw;
    const int tid = threadIdx.x;
    const size_t item = blockIdx.x;                                // (r, c) flattened
    const DayRow dr = day_row(S, C, N, start, item);
    const float* __restrict__ x = data + dr.trace;

    for (int p = tid; p < n_pad; p += PK_THREADS) {
        int i = p - shift;                                         // np.pad(mode="reflect"), shift <= n - 1
        i = i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i);
        row[p] = clipped_sample(x, dr.start + i, N);
    }
    __syncthreads();
    const int lo = nw > 2 ? 1 : 0, hi = nw > 2 ? nw - 2 : 0;       // the windows whose statistics survive
    for (int k = lo; k <= hi; ++k) {
        for (int l = tid; l < W; l += PK_THREADS) win[l] = row[k * shift + l];
        __syncthreads();
        float mean;
        float sd = block_std(win, W, tab, scratch, tid, &mean);    // (ends behind a barrier: win is free again)
        if (sd == 0.0f) sd = 1.0f;
        if (tid == 0) {
            w_mean[k] = mean;
            w_std[k] = sd;
        }
    }
    __syncthreads();

    const double first = nodes[0], last = nodes[nw - 1];
    OutT* __restrict__ o = out + item * (size_t)n;
    for (int i = tid; i < n; i += PK_THREADS) {
        const double t = (double)i;
        int j;
        bool at_node = true;
        if (t > last) j = nw - 1;
        else if (t < first) j = 0;
        else {
            int a = 0, b = nw;                                     // the nodes <= t are [0, a)
            while (a < b) {
                const int mid = (a + b) >> 1;
                if (nodes[mid] <= t) a = mid + 1;
                else b = mid;
            }
            j = a - 1;
            at_node = j == nw - 1 || nodes[j] == t;
        }
        const int k0 = j < lo ? lo : (j > hi ? hi : j);
        double m = (double)w_mean[k0], sd = (double)w_std[k0];
        if (!at_node) {
            const int k1 = j + 1 < lo ? lo : (j + 1 > hi ? hi : j + 1);
            const double x0 = nodes[j], dx = nodes[j + 1] - x0, dt = t - x0;
            const double slope_m = ((double)w_mean[k1] - m) / dx, slope_s = ((double)w_std[k1] - sd) / dx;
            m = slope_m * dt + m;
            sd = slope_s * dt + sd;
        }
        o[i] = (OutT)(((double)row[shift + i] - m) / sd);
    }
}

// exclusive prefix sum of v over the block's threads; *total = the sum.  Every thread calls it.
__device__ inline int block_exclusive_scan(int v, int* wave_total, int tid, int* total)
{
    const int lane = tid & 63, wave = tid >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    int base = 0, all = 0;
    for (int w = 0; w < PK_THREADS / 64; ++w) {
        if (w < wave) base += wave_total[w];
        all += wave_total[w];
    }
    *total = all;
    __syncthreads();                                               // (the next scan writes wave_total again)
    return base + incl - v;
}

// the midpoint of the plateau that the rise at i (1 <= i <= n - 2) opens, if a fall ends it; else -1
__device__ inline int peak_from_rise(const float* x, int n, int i)
{
    const float v = x[i];
    if (!(x[i - 1] < v)) return -1;
    int a = i + 1;
    while (a < n - 1 && x[a] == v) ++a;
    if (!(x[a] < v)) return -1;
    return (i + a - 1) >> 1;
}

// prominence and width of the peak at pk; false if either is too small, else the sample range of the pick
__device__ inline bool pick_window(const float* x, int n, int pk, double min_prominence, int* first, int* last)
{
    const float v = x[pk];
    int j = pk, left_base = pk, right_base = pk;
    float left_min = v, right_min = v;
    while (j >= 0 && x[j] <= v) {
        if (x[j] < left_min) {
            left_min = x[j];
            left_base = j;
        }
        --j;
    }
    j = pk;
    while (j <= n - 1 && x[j] <= v) {
        if (x[j] < right_min) {
            right_min = x[j];
            right_base = j;
        }
        ++j;
    }
    const double prominence = (double)v - (double)(left_min > right_min ? left_min : right_min);
    if (!(min_prominence <= prominence)) return false;
    const double h = (double)v - prominence * 0.5;
    j = pk;
    while (left_base < j && h < (double)x[j]) --j;
    double left_ip = (double)j;
    if ((double)x[j] < h) left_ip += (h - (double)x[j]) / ((double)x[j + 1] - (double)x[j]);
    j = pk;
    while (j < right_base && h < (double)x[j]) ++j;
    double right_ip = (double)j;
    if ((double)x[j] < h) right_ip -= (h - (double)x[j]) / ((double)x[j - 1] - (double)x[j]);
    if (!(1.0 <= right_ip - left_ip)) return false;
    *first = (int)left_ip;
    *last = (int)right_ip;
    return true;
}

__global__ __launch_bounds__(PK_THREADS) void find_picks_kernel(
    const float* __restrict__ proba, int n, double thr_even, double thr_odd, double prom_even, double prom_odd,
    int max_picks, int32_t* __restrict__ count, float* __restrict__ value, double* __restrict__ mean,
    double* __restrict__ spread, int32_t* __restrict__ index)
{
    extern __shared__ __align__(16) float pk_lds[];
    __shared__ int wave_total[PK_THREADS / 64];
    float* x = pk_lds;                                             // the series
    int* cand = (int*)(pk_lds + n);                                // candidate peaks, ascending: at most (n - 1) / 2
    const int tid = threadIdx.x;
    const size_t trace = blockIdx.x;
    const double thr = (trace & 1) ? thr_odd : thr_even, min_prominence = (trace & 1) ? prom_odd : prom_even;
    const float* __restrict__ src = proba + trace * (size_t)n;
    for (int i = tid; i < n; i += PK_THREADS) x[i] = src[i];
    __syncthreads();

    // 1. candidates of this thread's stretch [a, b) of the rises 1 .. n - 2
    const int per = (n + PK_THREADS - 1) / PK_THREADS;
    const int a = tid * per < 1 ? 1 : tid * per, b = (tid + 1) * per < n - 1 ? (tid + 1) * per : n - 1;
    int mine = 0;
    for (int i = a; i < b; ++i) {
        const int pk = peak_from_rise(x, n, i);
        if (pk >= 0 && (double)x[pk] >= thr) ++mine;
    }
    int n_cand;
    int slot = block_exclusive_scan(mine, wave_total, tid, &n_cand);
    for (int i = a; i < b; ++i) {
        const int pk = peak_from_rise(x, n, i);
        if (pk >= 0 && (double)x[pk] >= thr) cand[slot++] = pk;
    }
    __syncthreads();

    // 2. prominence and width: a candidate that fails becomes -1
    for (int q = tid; q < n_cand; q += PK_THREADS) {
        int first, last;
        if (!pick_window(x, n, cand[q], min_prominence, &first, &last)) cand[q] = -1;
    }
    __syncthreads();

    // 3. rank the survivors, write the first max_picks records
    const int cper = (n_cand + PK_THREADS - 1) / PK_THREADS;
    const int qa = tid * cper < n_cand ? tid * cper : n_cand, qb = qa + cper < n_cand ? qa + cper : n_cand;
    int kept = 0;
    for (int q = qa; q < qb; ++q) kept += cand[q] >= 0;
    int n_picks;
    int rank = block_exclusive_scan(kept, wave_total, tid, &n_picks);
    if (tid == 0) count[trace] = n_picks;
    const size_t rec = trace * (size_t)max_picks;
    for (int q = qa; q < qb; ++q) {
        const int pk = cand[q];
        if (pk < 0) continue;
        if (rank < max_picks) {
            int first = 0, last = 0;
            pick_window(x, n, pk, min_prominence, &first, &last);
            const int len = last - first + 1;
            const float* xs = x + first;
            const double s1 = np_sum<double>([=](int i) { return (double)(first + i) * (double)xs[i]; }, len);
            const double s0 = (double)np_sum<float>([=](int i) { return xs[i]; }, len);
            const double mu = s1 / s0;
            const double s2 = np_sum<double>([=](int i) {
                const double d = (double)(first + i) - mu;
                return d * d;
            }, len);
            value[rec + rank] = x[pk];
            mean[rec + rank] = mu;
            spread[rec + rank] = __dsqrt_rn(s2 / s0);
            index[rec + rank] = pk;
        }
        ++rank;
    }
    for (int k = n_picks + tid; k < max_picks; k += PK_THREADS) {  // (n_picks >= max_picks: nothing left over)
        value[rec + k] = __builtin_nanf("");
        mean[rec + k] = __builtin_nan("");
        spread[rec + k] = __builtin_nan("");
        index[rec + k] = -1;
    }
}

}  // namespace bpmf

using namespace bpmf;

extern "C" int bpmf_normalize_batch_dev(const float* d_data, size_t S, size_t C, size_t N, size_t n_rows,
                                        const int64_t* d_start_or_null, size_t n_samples, size_t window, size_t shift,
                                        const double* d_nodes, size_t n_windows, int out_f64, bpmf_stream_t stream_,
                                        void* d_out)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n_rows == 0) return 0;
    if (day_rows_refused("bpmf_normalize_batch_dev", false, !d_data || !d_nodes || !d_out, S, C, N, n_rows, set_error))
        return -1;
    if (window < 2 || window > (size_t)NP_CHUNK || shift < 1 || n_samples < 2 || shift > n_samples - 1 ||
        n_samples > (1u << 24)) {
        set_error("bpmf_normalize_batch_dev: need 2 <= window <= %d and 1 <= shift <= n_samples - 1 (n_samples=%zu "
                  "window=%zu shift=%zu)", NP_CHUNK, n_samples, window, shift);
        return -1;
    }
    const size_t n_pad = n_samples + 2 * shift;
    const size_t nw = n_pad >= window ? (n_pad - window) / shift + 1 : 0;
    if (nw < 2 || nw != n_windows) {
        set_error("bpmf_normalize_batch_dev: %zu samples hold %zu windows of %zu at shift %zu; need at least 2 and as "
                  "many nodes (%zu given)", n_samples, nw, window, shift, n_windows);
        return -1;
    }
    const size_t lds = (n_pad + window + 2 * nw) * sizeof(float);
    if (lds > PK_NORM_LDS_BYTES) {
        set_error("bpmf_normalize_batch_dev: n_samples + 2 shift + window + 2 n_windows = %zu floats; the row is staged "
                  "in LDS and at most %zu fit (n_samples=%zu window=%zu shift=%zu)", lds / sizeof(float),
                  PK_NORM_LDS_BYTES / sizeof(float), n_samples, window, shift);
        return -1;
    }
    LeafTable tab{};
    if (!list_leaves((int)window, tab)) {
        set_error("bpmf_normalize_batch_dev: the pairwise tree has more than %d leaves", NP_MAX_LEAVES);
        return -1;
    }
    const size_t n_items = n_rows * C, out_bytes = n_items * n_samples * (out_f64 ? sizeof(double) : sizeof(float));
    // option debug.poison_output (tests): an element the kernel skips comes back as NaN
    if (option(OPT_DEBUG_POISON_OUTPUT) != 0) BPMF_HIP_CHECK(hipMemsetAsync(d_out, 0xFF, out_bytes, stream));
    const dim3 grid((unsigned)n_items), block(PK_THREADS);
#define PK_LAUNCH(OUT_T)                                                                                              \
    do {                                                                                                               \
        auto kern = normalize_batch_kernel<OUT_T>;                                                                     \
        if (lds > 64 * 1024)   /* long rows: opt in to > 64 KB dynamic LDS */                                          \
            BPMF_HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,          \
                                               (int)PK_NORM_LDS_BYTES));                                               \
        kern<<<grid, block, lds, stream>>>(d_data, (int)S, (int)C, (long long)N, (const long long*)d_start_or_null,    \
                                           (int)n_samples, (int)window, (int)shift, (int)nw, d_nodes, tab,             \
                                           (OUT_T*)d_out);                                                             \
    } while (0)
    if (out_f64) PK_LAUNCH(double);
    else PK_LAUNCH(float);
#undef PK_LAUNCH
    BPMF_LAUNCH_CHECK();
    return 0;
}

extern "C" int bpmf_find_picks_dev(const float* d_proba, size_t n_traces, size_t n_samples, double threshold_even,
                                   double threshold_odd, size_t max_picks, bpmf_stream_t stream_, int32_t* d_count,
                                   float* d_value, double* d_mean, double* d_std, int32_t* d_index)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n_traces == 0) return 0;
    if (!d_proba || !d_count || !d_value || !d_mean || !d_std || !d_index) {
        set_error("bpmf_find_picks_dev: null pointer");
        return -1;
    }
    if (n_samples == 0 || n_samples > (size_t)PK_MAX_SERIES || max_picks == 0 || max_picks > (size_t)PK_MAX_PICKS ||
        n_traces > 0x7fffffffull || threshold_even != threshold_even || threshold_odd != threshold_odd) {
        set_error("bpmf_find_picks_dev: need 1 <= n_samples <= %d (the series is staged in LDS), 1 <= max_picks <= %d, "
                  "fewer than 2^31 series and thresholds that are numbers (n_samples=%zu max_picks=%zu series=%zu)",
                  PK_MAX_SERIES, PK_MAX_PICKS, n_samples, max_picks, n_traces);
        return -1;
    }
    if (option(OPT_DEBUG_POISON_OUTPUT) != 0) {
        const size_t slots = n_traces * max_picks;
        BPMF_HIP_CHECK(hipMemsetAsync(d_count, 0xFF, n_traces * sizeof(int32_t), stream));
        BPMF_HIP_CHECK(hipMemsetAsync(d_value, 0xFF, slots * sizeof(float), stream));
        BPMF_HIP_CHECK(hipMemsetAsync(d_mean, 0xFF, slots * sizeof(double), stream));
        BPMF_HIP_CHECK(hipMemsetAsync(d_std, 0xFF, slots * sizeof(double), stream));
        BPMF_HIP_CHECK(hipMemsetAsync(d_index, 0x7F, slots * sizeof(int32_t), stream));
    }
    const size_t lds = (n_samples + n_samples / 2 + 1) * sizeof(float);
    if (lds > 64 * 1024)
        BPMF_HIP_CHECK(hipFuncSetAttribute((const void*)find_picks_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)((PK_MAX_SERIES + PK_MAX_SERIES / 2 + 1) * sizeof(float))));
    // scipy's prominence=0.9 * threshold, the product taken in float64 as Python takes it
    find_picks_kernel<<<dim3((unsigned)n_traces), dim3(PK_THREADS), lds, stream>>>(
        d_proba, (int)n_samples, threshold_even, threshold_odd, 0.9 * threshold_even, 0.9 * threshold_odd,
        (int)max_picks, d_count, d_value, d_mean, d_std, d_index);
    BPMF_LAUNCH_CHECK();
    return 0;
}
