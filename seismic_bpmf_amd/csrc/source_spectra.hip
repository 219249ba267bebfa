// Propagation corrections, network-average spectra and the approximate moment magnitude of a day's events on the device
// (BPMF/spectrum.py: compute_signal_to_noise_ratio :601-648, correct_geometrical_spreading :200-227, correct_attenuation
// :229-256, compute_network_average_spectrum :258-386, approximate_moment_magnitude :1341-1496; the definitions are
// postprocess.source_spectra_host and postprocess.approximate_moment_magnitude_host).  One call serves one phase of E
// events; a workgroup of one wave takes one event, so an event's bits do not depend on the batch.
//   ss_average_kernel  stages 1-3.  Lanes over the event's (channel, bin) elements: the SNR and the corrected value
//                      fl(fl(x g) a), g = fl(fl(c r_m) / radiation), a = exp(fl(fl(fl(pi tt) f) / q)) -- two roundings,
//                      geometry first, nothing fused.  Then lanes over bins, the channels of a bin one after the other
//                      in channel order as np.ma adds them: the count, the rule of the least count, log10's domain, the
//                      sum (0 for a masked channel), the mean, the deviations' sum, and for the median a rank count over
//                      the bin's column in LDS ((channels, 64) doubles, masked = +inf; an unmasked NaN gives NaN before
//                      any comparison is made, so nothing waits on one).
//   ss_mw_kernel       stage 4.  Lanes over channels: the lowest valid bands (their median from a fixed network of
//                      compare-exchanges in registers) or the SNR-weighted log-mean (np_order.h sums over the bands); then, in LDS,
//                      the ranks of the float32 SNRs (ties by index) for _snr_based_weights, the ranks of the event's
//                      epicentral distances for np.percentile's two linear interpolations, and lane 0's sums over the
//                      present channels in NumPy's order.  Every loop has a bound that depends on sizes only.
// No workspace, no atomics, plain vector stores; every element of the outputs of the stages asked for is written.
#include "common.h"
#include <cmath>
#include "np_order.h"
#include "../../include/bpmf_hip.h"

namespace bpmf {

constexpr int SS_MAX_CHANNELS = 256;                    // S * C of an event: the median's column (256 x 64 x 8 = 128 KB)
constexpr int SS_MAX_FREQUENCIES = 1024;                // as bpmf_fft_spectrum_dev's targets
constexpr int SS_MAX_BANDS = 8;                         // num_averaging_bands
constexpr int SS_LANES = 64;
constexpr unsigned SS_SNR = 1, SS_CORRECT = 2, SS_AVERAGE = 4, SS_MW = 8;
constexpr double SS_LOG_OF_10 = 2.302585092994046;      // np.log(10.0)

struct SsCall {
    const double *signal, *noise;                       // (E, NC, F)
    const unsigned char *valid, *noise_valid;           // (E, S)
    const double *dist, *epi, *tt;                      // (E, S)
    const double* loc_err;                              // (E)
    const double *freq, *q;                             // (F)
    double *corrected, *snr;                            // (E, NC, F): written by stages 2 and 1, read by 3 and 4
    double *average, *std;                              // (E, F)
    unsigned char* mask;                                // (E, F)
    int* num_valid;                                     // (E, F)
    unsigned char* used;                                // (E, S)
    double *mw, *log10_m0;                              // (E)
    double* measured;                                   // (E, NC)
    float *weights, *msnr;                              // (E, NC)
    double geometry_c, radiation, snr_threshold, max_err_pct, scaling;
    float thr32, clip32, wmax32;
    int S, C, F, NC, min_num_valid, average_log, median, n_bands, first_high, max_bad;
    unsigned flags;
};

__device__ inline bool ss_nan(double v) { return v != v; }
__device__ inline double ss_quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ inline double ss_inf() { return __longlong_as_double(0x7ff0000000000000ll); }
// np.minimum / np.maximum: a NaN wins
__device__ inline double ss_min(double a, double b) { return ss_nan(a) ? a : (ss_nan(b) ? b : (a < b ? a : b)); }
__device__ inline double ss_max(double a, double b) { return ss_nan(a) ? a : (ss_nan(b) ? b : (a > b ? a : b)); }
__device__ inline float ss_minf(float a, float b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }
// a sorts before b as np.sort orders them: NaN last
__device__ inline bool ss_before(double a, double b) { return ss_nan(b) ? !ss_nan(a) : a < b; }

__global__ __launch_bounds__(SS_LANES) void ss_average_kernel(const SsCall c)
{
    extern __shared__ double ss_column[];               // (NC, 64) when the median is asked for
    __shared__ unsigned char s_used[SS_MAX_CHANNELS];   // per station
    const int e = blockIdx.x, tid = threadIdx.x;
    const size_t base = (size_t)e * c.NC * c.F;

    for (int i = tid; i < c.NC * c.F; i += SS_LANES) {
        const int ch = i / c.F, f = i - ch * c.F;
        const size_t es = (size_t)e * c.S + ch / c.C;
        const bool present = c.valid[es] != 0;
        if (c.flags & SS_SNR) {
            const double x = fabs(c.signal[base + i]), z = fabs(c.noise[base + i]);
            const bool keep = present && c.noise_valid[es] != 0 && !(x == 0.0 && z == 0.0);
            c.snr[base + i] = keep ? x / z : 0.0;
        }
        if (c.flags & SS_CORRECT) {
            const double geometry = c.geometry_c * (1000.0 * c.dist[es]) / c.radiation;
            const double att = exp(M_PI * c.tt[es] * c.freq[f] / c.q[f]);
            const double first = c.signal[base + i] * geometry;
            c.corrected[base + i] = present ? first * att : 0.0;
        }
    }
    if (!(c.flags & SS_AVERAGE)) return;
    for (int s = tid; s < c.S; s += SS_LANES) {
        const size_t es = (size_t)e * c.S + s;
        const double pct = 100.0 * (c.loc_err[e] / c.dist[es]);
        const unsigned char u = c.valid[es] != 0 && !(pct > c.max_err_pct);
        s_used[s] = u;
        c.used[es] = u;
    }
    __syncthreads();                                    // the block's own stores to corrected and snr, and s_used

    const double* snr = c.snr + base;
    const double* val = c.corrected + base;
    for (int f = tid; f < c.F; f += SS_LANES) {
        int num_valid = 0, n_used = 0;
        for (int ch = 0; ch < c.NC; ++ch) {
            if (!s_used[ch / c.C]) continue;
            num_valid += !(snr[(size_t)ch * c.F + f] < c.snr_threshold);
            ++n_used;
        }
        const bool discard = num_valid < c.min_num_valid;
        double sum = 0.0;
        int count = 0, k = 0;
        bool any_nan = false;
        for (int ch = 0; ch < c.NC; ++ch) {
            if (!s_used[ch / c.C]) continue;
            const double x = val[(size_t)ch * c.F + f];
            bool m = snr[(size_t)ch * c.F + f] < c.snr_threshold || discard;
            double v = x;
            if (c.average_log) {                        // np.ma.log10: its domain, and a result that is not finite
                v = log10(x);
                m = m || x <= 0.0 || !(v - v == 0.0);
            }
            const double filled = m ? 0.0 : v;
            sum = k == 0 ? filled : sum + filled;
            count += !m;
            any_nan = any_nan || (!m && ss_nan(v));
            if (c.median) ss_column[k * SS_LANES + tid] = m || ss_nan(v) ? ss_inf() : v;
            ++k;
        }
        const double mean = sum * 1.0 / count;
        double dsum = 0.0;
        k = 0;
        for (int ch = 0; ch < c.NC; ++ch) {
            if (!s_used[ch / c.C]) continue;
            const double x = val[(size_t)ch * c.F + f];
            bool m = snr[(size_t)ch * c.F + f] < c.snr_threshold || discard;
            double v = x;
            if (c.average_log) {                        // np.ma.log10: its domain, and a result that is not finite
                v = log10(x);
                m = m || x <= 0.0 || !(v - v == 0.0);
            }
            const double d = m ? 0.0 : v - mean;
            const double dd = d * d;
            dsum = k == 0 ? dd : dsum + dd;
            ++k;
        }
        double centre = mean;
        if (c.median && n_used > 0) {
            const int hi = count / 2 < n_used - 1 ? count / 2 : n_used - 1;
            const int lo = (count & 1) ? hi : (hi > 0 ? hi - 1 : 0);
            double a = 0.0, b = 0.0;
            for (int i = 0; i < n_used; ++i) {          // the rank of every entry: ties by index
                const double vi = ss_column[i * SS_LANES + tid];
                int rank = 0;
                for (int j = 0; j < n_used; ++j) {
                    const double vj = ss_column[j * SS_LANES + tid];
                    rank += vj < vi || (vj == vi && j < i);
                }
                if (rank == lo) a = vi;
                if (rank == hi) b = vi;
            }
            centre = any_nan ? ss_quiet_nan() : (a + b) / 2.0;
        }
        const double value = c.average_log ? exp(centre * SS_LOG_OF_10) : centre;
        const double variance = dsum / count;
        // np.ma's division masks a quotient that is not finite: the mean (not the median) and the variance
        const bool masked = count == 0 || (!c.median && !(mean - mean == 0.0));
        const size_t o = (size_t)e * c.F + f;
        c.average[o] = masked ? ss_quiet_nan() : value;
        // (np.ma.var under a masked mean: the deviations are masked, their sum is 0, its own mask is the counts')
        c.std[o] = count == 0 ? ss_quiet_nan()
                              : (!(mean - mean == 0.0) ? 0.0
                                                       : (!(variance - variance == 0.0) ? ss_quiet_nan() : sqrt(variance)));
        c.mask[o] = masked;
        c.num_valid[o] = num_valid;
    }
}

__global__ __launch_bounds__(SS_LANES) void ss_mw_kernel(const SsCall c)
{
    __shared__ double s_measured[SS_MAX_CHANNELS], s_sorted[SS_MAX_CHANNELS], s_peak[SS_MAX_CHANNELS];
    __shared__ float s_snr[SS_MAX_CHANNELS], s_weight[SS_MAX_CHANNELS];
    __shared__ int s_list[SS_MAX_CHANNELS];
    const int e = blockIdx.x, tid = threadIdx.x;
    const size_t base = (size_t)e * c.NC * c.F;
    const unsigned char* present = c.valid + (size_t)e * c.S;
    const double* epi = c.epi + (size_t)e * c.S;

    // 1. a channel's measurement and its float32 SNR
    for (int ch = tid; ch < c.NC; ch += SS_LANES) {
        double disp = ss_quiet_nan();
        float m32 = 0.0f;
        if (present[ch / c.C]) {
            const double* r = c.snr + base + (size_t)ch * c.F;
            const double* x = c.corrected + base + (size_t)ch * c.F;
            double chosen[SS_MAX_BANDS];
            int n = 0;
            bool any_nan = false;
#pragma unroll
            for (int j = 0; j < SS_MAX_BANDS; ++j) chosen[j] = ss_inf();
            for (int f = 0; f < c.F; ++f) {
                if (n < c.n_bands && r[f] > c.snr_threshold) {          // the lowest valid bands
                    const double v = x[f];
                    any_nan = any_nan || ss_nan(v);
#pragma unroll
                    for (int j = 0; j < SS_MAX_BANDS; ++j)
                        if (j == n) chosen[j] = v;
                    ++n;
                }
            }
            if (n > 0) {
#pragma unroll
                for (int pass = 0; pass < SS_MAX_BANDS - 1; ++pass) {   // ascending; the unused entries (+inf) last
#pragma unroll
                    for (int j = 0; j + 1 < SS_MAX_BANDS - pass; ++j) {
                        const double a = chosen[j], b = chosen[j + 1];
                        const bool swap = b < a;
                        chosen[j] = swap ? b : a;
                        chosen[j + 1] = swap ? a : b;
                    }
                }
                double lo = chosen[0], hi = chosen[0];
#pragma unroll
                for (int j = 0; j < SS_MAX_BANDS; ++j) {
                    if (j == (n - 1) / 2) lo = chosen[j];
                    if (j == n / 2) hi = chosen[j];
                }
                disp = n == 1 ? chosen[0] : (any_nan ? ss_quiet_nan() : (lo + hi) / 2.0);
                m32 = (float)c.snr_threshold;
            } else {
                const int first = c.first_high, count = c.F - c.first_high;
                const auto zero_nan = [](double v) { return ss_nan(v) ? 0.0 : v; };
                double total = np_sum<double>([&](int i) { return zero_nan(r[first + i]); }, count);
                total = total == 0.0 ? 1.0 : total;
                const double logs = np_sum<double>(
                    [&](int i) { return zero_nan(r[first + i] * log10(x[first + i])); }, count);
                const double squares = np_sum<double>(
                    [&](int i) { return zero_nan(r[first + i] * r[first + i]); }, count);
                disp = pow(10.0, logs / total);
                m32 = (float)(squares / total);
            }
            if (disp == 0.0) m32 = 0.0f;
        }
        s_measured[ch] = disp;
        s_snr[ch] = m32;
        c.measured[(size_t)e * c.NC + ch] = disp;
        c.msnr[(size_t)e * c.NC + ch] = m32;
    }
    // 2. the event's epicentral distances in np.sort's order
    for (int s = tid; s < c.S; s += SS_LANES) {
        const double v = epi[s];
        int rank = 0;
        for (int j = 0; j < c.S; ++j) {
            const double w = epi[j];
            rank += ss_before(w, v) || (!ss_before(v, w) && j < s);
        }
        s_sorted[rank] = v;
    }
    __syncthreads();
    // np.percentile(..., 25) and (..., 75), method "linear": virtual index q (n - 1), NumPy's two-sided lerp
    double bound[2];
    for (int k = 0; k < 2; ++k) {
        const double q = k == 0 ? 0.25 : 0.75;
        const double vi = c.S * q + (1.0 - q) - 1.0;
        const int lo = (int)floor(vi);
        const int hi = lo + 1 < c.S ? lo + 1 : c.S - 1;
        const double t = vi - lo, a = s_sorted[lo], b = s_sorted[hi], diff = b - a;
        double v = t >= 0.5 ? b - diff * (1.0 - t) : a + diff * t;
        if (ss_nan(s_sorted[c.S - 1])) v = ss_quiet_nan();
        bound[k] = v;
    }
    // 3. _snr_based_weights among the present channels, times the reciprocal of the clipped distance
    for (int ch = tid; ch < c.NC; ch += SS_LANES) {
        float w = 0.0f;
        if (present[ch / c.C]) {
            const float m = s_snr[ch];
            int n_channels = 0, n_good = 0, rank = 0;
            for (int j = 0; j < c.NC; ++j) {
                if (!present[j / c.C]) continue;
                const float o = s_snr[j];
                ++n_channels;
                n_good += o >= c.thr32;
                rank += o < m || (o == m && j < ch);
            }
            w = ss_minf(ss_minf(m, c.clip32), c.wmax32);
            if (n_good >= c.max_bad) {
                if (m < c.thr32) w = 0.0f;
            } else if (rank < n_channels - c.max_bad) {
                w = 0.0f;
            }
            const double clipped = ss_min(ss_max(epi[ch / c.C], bound[0]), bound[1]);
            w = (float)((double)w * (1.0 / clipped));
        }
        s_weight[ch] = w;
        c.weights[(size_t)e * c.NC + ch] = w;
        s_peak[ch] = w > 0.0f ? log10(s_measured[ch]) * (double)w : 0.0;
    }
    __syncthreads();
    // 4. the two sums over the present channels, in NumPy's order
    if (tid == 0) {
        int n = 0;
        for (int ch = 0; ch < c.NC; ++ch)
            if (present[ch / c.C]) s_list[n++] = ch;
        double m0 = ss_quiet_nan();
        if (n > 0) {
            const double peaks = np_sum<double>([&](int i) { return s_peak[s_list[i]]; }, n);
            const float weights = np_sum<float>([&](int i) { return s_weight[s_list[i]]; }, n);
            m0 = peaks / (double)weights;
        }
        c.log10_m0[e] = m0;
        c.mw[e] = c.scaling * (m0 - 9.1);
    }
}

}  // namespace bpmf

using namespace bpmf;

extern "C" int bpmf_source_spectra_dev(const double* d_signal, const double* d_noise, const unsigned char* d_valid,
                                       const unsigned char* d_noise_valid, const double* d_dist,
                                       const double* d_epicentral_dist, const double* d_travel_time,
                                       const double* d_location_err, const double* d_frequencies, const double* d_q,
                                       size_t E, size_t S, size_t C, size_t F, unsigned flags,
                                       double geometry_constant, double radiation, double snr_threshold,
                                       double max_relative_distance_err_pct, int min_num_valid, int average_log,
                                       int reduce_median, int num_averaging_bands, size_t first_high_band,
                                       double magnitude_log_moment_scaling, double weight_max,
                                       int max_num_bad_measurements, bpmf_stream_t stream_, double* d_corrected,
                                       double* d_snr, double* d_average, unsigned char* d_mask, double* d_std,
                                       int* d_num_valid, unsigned char* d_used, double* d_mw_star, double* d_log10_m0,
                                       double* d_measured_disp, float* d_weights, float* d_measurement_snr)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (E == 0) return 0;
    if (flags == 0 || (flags & ~(SS_SNR | SS_CORRECT | SS_AVERAGE | SS_MW))) {
        set_error("bpmf_source_spectra_dev: flags = %u; bits 1 (SNR), 2 (correction), 4 (average), 8 (Mw*)", flags);
        return -1;
    }
    const bool snr = flags & SS_SNR, correct = flags & SS_CORRECT, average = flags & SS_AVERAGE, mw = flags & SS_MW;
    // d_corrected: written by stage 2, read by 4 and 8; d_snr: written by stage 1, read by 4 and 8
    if (!d_valid || ((correct || average || mw) && !d_corrected) || ((snr || average || mw) && !d_snr) ||
        ((snr || correct) && !d_signal) ||
        (snr && (!d_noise || !d_noise_valid)) ||
        (correct && (!d_dist || !d_travel_time || !d_frequencies || !d_q)) ||
        (average && (!d_dist || !d_location_err || !d_average || !d_mask || !d_std || !d_num_valid || !d_used)) ||
        (mw && (!d_epicentral_dist || !d_mw_star || !d_log10_m0 || !d_measured_disp || !d_weights ||
                !d_measurement_snr))) {
        set_error("bpmf_source_spectra_dev: null pointer");
        return -1;
    }
    if (S == 0 || C == 0 || F == 0 || S > (size_t)SS_MAX_CHANNELS || C > (size_t)SS_MAX_CHANNELS ||
        S * C > (size_t)SS_MAX_CHANNELS || F > (size_t)SS_MAX_FREQUENCIES) {
        set_error("bpmf_source_spectra_dev: need 1 .. %d channels (S=%zu C=%zu) and 1 .. %d frequencies (F=%zu)",
                  SS_MAX_CHANNELS, S, C, SS_MAX_FREQUENCIES, F);
        return -1;
    }
    if (E > 0x7fffffffull / (S * C * F)) {
        set_error("bpmf_source_spectra_dev: %zu events x %zu channels x %zu frequencies; fewer than 2^31 values fit", E,
                  S * C, F);
        return -1;
    }
    if (mw && (num_averaging_bands < 1 || num_averaging_bands > SS_MAX_BANDS || first_high_band > F ||
               max_num_bad_measurements < 0)) {
        set_error("bpmf_source_spectra_dev: need num_averaging_bands 1 .. %d (%d), first_high_band <= F (%zu) and "
                  "max_num_bad_measurements >= 0 (%d)", SS_MAX_BANDS, num_averaging_bands, first_high_band,
                  max_num_bad_measurements);
        return -1;
    }
    const size_t NC = S * C;
    // option debug.poison_output (tests): an element the kernels skip comes back as NaN / 255 / -1
    if (option(OPT_DEBUG_POISON_OUTPUT) != 0) {
        if (snr) BPMF_HIP_CHECK(hipMemsetAsync(d_snr, 0xFF, E * NC * F * sizeof(double), stream));
        if (correct) BPMF_HIP_CHECK(hipMemsetAsync(d_corrected, 0xFF, E * NC * F * sizeof(double), stream));
        if (average) {
            BPMF_HIP_CHECK(hipMemsetAsync(d_average, 0xFF, E * F * sizeof(double), stream));
            BPMF_HIP_CHECK(hipMemsetAsync(d_std, 0xFF, E * F * sizeof(double), stream));
            BPMF_HIP_CHECK(hipMemsetAsync(d_mask, 0xFF, E * F, stream));
            BPMF_HIP_CHECK(hipMemsetAsync(d_num_valid, 0xFF, E * F * sizeof(int), stream));
            BPMF_HIP_CHECK(hipMemsetAsync(d_used, 0xFF, E * S, stream));
        }
        if (mw) {
            BPMF_HIP_CHECK(hipMemsetAsync(d_mw_star, 0xFF, E * sizeof(double), stream));
            BPMF_HIP_CHECK(hipMemsetAsync(d_log10_m0, 0xFF, E * sizeof(double), stream));
            BPMF_HIP_CHECK(hipMemsetAsync(d_measured_disp, 0xFF, E * NC * sizeof(double), stream));
            BPMF_HIP_CHECK(hipMemsetAsync(d_weights, 0xFF, E * NC * sizeof(float), stream));
            BPMF_HIP_CHECK(hipMemsetAsync(d_measurement_snr, 0xFF, E * NC * sizeof(float), stream));
        }
    }
    SsCall call{};
    call.signal = d_signal, call.noise = d_noise, call.valid = d_valid, call.noise_valid = d_noise_valid;
    call.dist = d_dist, call.epi = d_epicentral_dist, call.tt = d_travel_time, call.loc_err = d_location_err;
    call.freq = d_frequencies, call.q = d_q;
    call.corrected = d_corrected, call.snr = d_snr, call.average = d_average, call.std = d_std, call.mask = d_mask;
    call.num_valid = d_num_valid, call.used = d_used, call.mw = d_mw_star, call.log10_m0 = d_log10_m0;
    call.measured = d_measured_disp, call.weights = d_weights, call.msnr = d_measurement_snr;
    call.geometry_c = geometry_constant, call.radiation = radiation, call.snr_threshold = snr_threshold;
    call.max_err_pct = max_relative_distance_err_pct, call.scaling = magnitude_log_moment_scaling;
    call.thr32 = (float)snr_threshold, call.clip32 = (float)(1.001 * snr_threshold), call.wmax32 = (float)weight_max;
    call.S = (int)S, call.C = (int)C, call.F = (int)F, call.NC = (int)NC;
    call.min_num_valid = min_num_valid, call.average_log = average_log ? 1 : 0, call.median = reduce_median ? 1 : 0;
    call.n_bands = num_averaging_bands, call.first_high = (int)first_high_band;
    call.max_bad = max_num_bad_measurements;
    call.flags = flags;
    if (snr || correct || average) {
        const size_t lds = average && reduce_median ? NC * SS_LANES * sizeof(double) : 0;
        if (lds > 64 * 1024)   // a long column: opt in to > 64 KB dynamic LDS
            BPMF_HIP_CHECK(hipFuncSetAttribute((const void*)ss_average_kernel,
                                               hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)(SS_MAX_CHANNELS * SS_LANES * sizeof(double))));
        ss_average_kernel<<<dim3((unsigned)E), dim3(SS_LANES), lds, stream>>>(call);
        BPMF_LAUNCH_CHECK();
    }
    if (mw) {
        ss_mw_kernel<<<dim3((unsigned)E), dim3(SS_LANES), 0, stream>>>(call);
        BPMF_LAUNCH_CHECK();
    }
    return 0;
}
