// Brune / Boatwright fits of a day's network-average source spectra on the device (BPMF/spectrum.py:
// fit_average_spectrum :729-849 with log=True, the below-fc gate, stress_drop_circular_crack :1249-1287; the definition is
// postprocess.fit_source_spectra_host).  The answer is the exact weighted least-squares minimum, not where SciPy's
// curve_fit stops: in log space the model a - g(f / fc) is linear in a = log10 Omega_0, so with u = ln fc the problem is
// the minimum over u of the profile cost P(u) = 1/2 sum w^2 (y + g - a(u))^2, a(u) = sum w^2 (y + g) / sum w^2.
//   fit_kernel   a workgroup of one wave takes one event, so an event's bits do not depend on the batch.  The unmasked
//                bins go to LDS in bin order (a ballot and a prefix count per 64 bins): y = log10(average), w^2, x and
//                ln x.  Then BPMF_FIT_SCAN_POINTS values of u over [ln(fc0 / 1e3), ln(fc0 1e3)], 16 per lane, each cost
//                two sequential float64 sums over the bins in bin order; the wave's lowest cost, ties to the lowest
//                index, a NaN as +inf; BPMF_FIT_ZOOM_ROUNDS rounds of one point per lane on the bracket of the two
//                neighbours; BPMF_FIT_NEWTON_STEPS Newton steps on the analytic P'(u) and P''(u), clamped to the last
//                bracket, the same on every lane; the 2 x 2 covariance in closed form.
// Every loop has a bound that depends on sizes and constants only; no comparison that a loop waits on reads a value
// that may be NaN.  No workspace, no atomics, plain vector stores; every element of every output is written.
#include "common.h"
#include <cmath>
#include "../../include/bpmf_hip.h"

namespace bpmf {

constexpr int FIT_MAX_FREQUENCIES = 1024;               // as bpmf_source_spectra_dev
constexpr int FIT_LANES = 64;
constexpr int FIT_SCAN = BPMF_FIT_SCAN_POINTS, FIT_ZOOM = BPMF_FIT_ZOOM_POINTS;
constexpr double FIT_LOG_OF_10 = 2.302585092994046;     // np.log(10.0)
constexpr double FIT_VR = 0.9 * 3500.0;                 // vr_vs_ratio * vs_m_per_s, the reference's defaults
static_assert(FIT_SCAN % FIT_LANES == 0 && FIT_ZOOM == FIT_LANES, "lanes over scan points; one zoom point per lane");

struct FitCall {
    const double* average;                              // (E, F)
    const unsigned char* mask;                          // (E, F)
    const int* num_valid;                               // (E, F)
    const double* freq;                                 // (F)
    double *m0, *fc, *mw, *m0_err, *fc_err, *cost, *stress;     // (E)
    int* n_valid;                                       // (E)
    unsigned char *success, *at_bound, *reason;         // (E)
    double n, crack_constant, min_fraction, min_fraction_below;
    int F, weighted;
};

struct FitBins {
    const double *y, *w2, *ln_x;
    int M;
    double n, sw;
};

__device__ inline double fit_quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ inline double fit_inf() { return __longlong_as_double(0x7ff0000000000000ll); }
__device__ inline bool fit_finite(double v) { return v - v == 0.0; }

// P(u) and a(u): two sums over the bins, one term after the other
__device__ inline double fit_cost(const FitBins& b, double u, double* a_out)
{
    const double scale = 2.0 / b.n;
    double sum = 0.0;
    for (int j = 0; j < b.M; ++j) {
        const double g = scale * log10(1.0 + exp(b.n * (b.ln_x[j] - u)));
        const double term = b.w2[j] * (b.y[j] + g);
        sum = j == 0 ? term : sum + term;
    }
    const double a = sum / b.sw;
    double cost = 0.0;
    for (int j = 0; j < b.M; ++j) {
        const double g = scale * log10(1.0 + exp(b.n * (b.ln_x[j] - u)));
        const double rho = (b.y[j] + g) - a;
        const double term = b.w2[j] * rho * rho;
        cost = j == 0 ? term : cost + term;
    }
    *a_out = a;
    return 0.5 * cost;
}

// P'(u), P''(u), the centred moment sum w^2 (g' - a')^2 and the plain one sum w^2 g'^2
__device__ inline void fit_derivatives(const FitBins& b, double u, double* p1, double* p2, double* centred, double* plain)
{
    const double scale = 2.0 / b.n, k1 = -(2.0 / FIT_LOG_OF_10), k2 = 2.0 * b.n / FIT_LOG_OF_10;
    double sz = 0.0, s1 = 0.0;
    for (int j = 0; j < b.M; ++j) {
        const double d = b.ln_x[j] - u;
        const double g = scale * log10(1.0 + exp(b.n * d));
        const double t = 1.0 / (1.0 + exp(-(b.n * d)));
        const double tz = b.w2[j] * (b.y[j] + g), t1 = b.w2[j] * (k1 * t);
        sz = j == 0 ? tz : sz + tz;
        s1 = j == 0 ? t1 : s1 + t1;
    }
    const double a = sz / b.sw, a1 = s1 / b.sw;
    double q1 = 0.0, qc = 0.0, q2 = 0.0, qp = 0.0;
    for (int j = 0; j < b.M; ++j) {
        const double d = b.ln_x[j] - u;
        const double g = scale * log10(1.0 + exp(b.n * d));
        const double t = 1.0 / (1.0 + exp(-(b.n * d)));
        const double g1 = k1 * t, g2 = k2 * (t * (1.0 - t));
        const double rho = (b.y[j] + g) - a, c1 = g1 - a1;
        const double t1 = b.w2[j] * rho * c1, tc = b.w2[j] * c1 * c1, t2 = b.w2[j] * rho * g2, tp = b.w2[j] * g1 * g1;
        q1 = j == 0 ? t1 : q1 + t1;
        qc = j == 0 ? tc : qc + tc;
        q2 = j == 0 ? t2 : q2 + t2;
        qp = j == 0 ? tp : qp + tp;
    }
    *p1 = q1, *p2 = qc + q2, *centred = qc, *plain = qp;
}

// the k-th of `count` points from lo to hi, both ends exact
__device__ inline double fit_point(double lo, double hi, int k, int count)
{
    return k == count - 1 ? hi : lo + (double)k * ((hi - lo) / (double)(count - 1));
}

// the wave's lowest cost, ties to the lowest index (every lane gets the index)
__device__ inline int fit_wave_lowest(double cost, int index)
{
#pragma unroll
    for (int off = FIT_LANES / 2; off >= 1; off >>= 1) {
        const double other = __shfl_xor(cost, off, FIT_LANES);
        const int other_index = __shfl_xor(index, off, FIT_LANES);
        const bool take = other < cost || (other == cost && other_index < index);
        cost = take ? other : cost;
        index = take ? other_index : index;
    }
    return index;
}

__global__ __launch_bounds__(FIT_LANES) void fit_kernel(const FitCall c)
{
    __shared__ double s_y[FIT_MAX_FREQUENCIES], s_w2[FIT_MAX_FREQUENCIES], s_x[FIT_MAX_FREQUENCIES],
        s_ln_x[FIT_MAX_FREQUENCIES];
    __shared__ double s_first;
    const int e = blockIdx.x, tid = threadIdx.x;
    const double* average = c.average + (size_t)e * c.F;
    const unsigned char* mask = c.mask + (size_t)e * c.F;
    const int* num_valid = c.num_valid + (size_t)e * c.F;

    // the mean of num_valid over ALL bins: integers, so exact in any order
    long long total = 0;
    for (int f = tid; f < c.F; f += FIT_LANES) total += num_valid[f];
#pragma unroll
    for (int off = FIT_LANES / 2; off >= 1; off >>= 1) total += __shfl_xor(total, off, FIT_LANES);
    const double mean = (double)total / (double)c.F;

    // the unmasked bins in bin order
    int M = 0;
    bool finite = true;
    for (int base = 0; base < c.F; base += FIT_LANES) {
        const int f = base + tid;
        const bool keep = f < c.F && mask[f] == 0;
        const unsigned long long votes = __ballot(keep);
        if (keep) {
            const int at = M + __popcll(votes & ((1ull << tid) - 1ull));
            const double v = average[f], x = c.freq[f];
            const double y = log10(v);
            const double w = c.weighted ? 1.0 / (1.0 + exp(-(((double)num_valid[f] - mean) / mean))) : 1.0;
            s_y[at] = y, s_w2[at] = w * w, s_x[at] = x, s_ln_x[at] = log(x);
            finite = finite && fit_finite(y) && fit_finite(w);
            if (at == 0) s_first = v;
        }
        M += __popcll(votes);
    }
    __syncthreads();
    finite = __ballot(!finite) == 0ull;

    double out[7];                                      // M0, fc, Mw, M0_err, fc_err, cost, stress drop
#pragma unroll
    for (int k = 0; k < 7; ++k) out[k] = fit_quiet_nan();
    int reason = 0;
    bool at_bound = false;
    if (M == 0) reason = 1;
    else if ((double)M / (double)c.F < c.min_fraction) reason = 2;
    else if (!finite) reason = 5;

    double lo = 0.0, hi = 0.0;
    if (reason == 0) {                                  // fc_circular_crack(moment_to_magnitude(Omega_0)), the P constant
        const double mw0 = 2.0 / 3.0 * (log10(s_first) - 9.1);
        const double radius = pow((7.0 / 16.0) * (pow(10.0, 3.0 / 2.0 * mw0 + 9.1) / 1.0e6), 1.0 / 3.0);
        const double fc0 = (2.23 * FIT_VR) / (2.0 * M_PI * radius);
        lo = log(fc0 / BPMF_FIT_BOUND_FACTOR), hi = log(fc0 * BPMF_FIT_BOUND_FACTOR);
        if (!fit_finite(lo) || !fit_finite(hi)) reason = 5;
    }
    if (reason == 0) {                                  // (the same on every lane: the branch is the wave's)
        FitBins b{s_y, s_w2, s_ln_x, M, c.n, 0.0};
        for (int j = 0; j < M; ++j) b.sw = j == 0 ? s_w2[0] : b.sw + s_w2[j];

        double a = lo, z = hi, unused;
        int count = FIT_SCAN;
        double u = lo;
        for (int round = 0; round < 1 + BPMF_FIT_ZOOM_ROUNDS; ++round) {
            double best = fit_inf();
            int best_index = count;
            for (int k = tid; k < count; k += FIT_LANES) {
                double cost = fit_cost(b, fit_point(a, z, k, count), &unused);
                cost = cost != cost ? fit_inf() : cost;
                if (cost < best || best_index == count) best = cost, best_index = k;
            }
            const int i = fit_wave_lowest(best, best_index);
            const double na = fit_point(a, z, i > 0 ? i - 1 : 0, count);
            const double nz = fit_point(a, z, i + 1 < count ? i + 1 : count - 1, count);
            u = fit_point(a, z, i, count);
            a = na, z = nz;
            count = FIT_ZOOM;
        }
        double p1, p2, centred, plain;
        for (int step = 0; step < BPMF_FIT_NEWTON_STEPS; ++step) {
            fit_derivatives(b, u, &p1, &p2, &centred, &plain);
            const double delta = p1 / p2;
            if (p2 > 0.0 && fit_finite(delta)) {
                const double next = u - delta;
                u = next < a ? a : (next > z ? z : next);
            }
        }
        double log_m0;
        const double cost = fit_cost(b, u, &log_m0);
        fit_derivatives(b, u, &p1, &p2, &centred, &plain);
        const double m0 = pow(10.0, log_m0), fc = exp(u);
        const double mw = 2.0 / 3.0 * (log10(m0) - 9.1);
        const double radius = c.crack_constant * FIT_VR / (2.0 * M_PI * fc);
        const double stress = 7.0 / 16.0 * pow(10.0, 3.0 / 2.0 * mw + 9.1) / pow(radius, 3.0);
        if (!(fit_finite(m0) && fit_finite(fc) && fit_finite(cost) && fit_finite(mw) && fit_finite(stress))) {
            reason = 5;
        } else {
            double cov_a = fit_inf(), cov_u = fit_inf();
            if (M > 2) {
                const double s2 = 2.0 * cost / (double)(M - 2);
                cov_a = s2 * plain / (b.sw * centred);
                cov_u = s2 / centred;
            }
            out[0] = m0, out[1] = fc, out[2] = mw, out[5] = cost, out[6] = stress;
            out[3] = (m0 * FIT_LOG_OF_10) * sqrt(cov_a);
            out[4] = fc * sqrt(cov_u);
            at_bound = u == lo || u == hi;
            int below = 0;
            for (int j = 0; j < M; ++j) below += s_x[j] < fc;
            if (at_bound) reason = 4;
            else if ((double)below / (double)c.F < c.min_fraction_below) reason = 3;
        }
    }
    if (tid == 0) {
        c.m0[e] = out[0], c.fc[e] = out[1], c.mw[e] = out[2], c.m0_err[e] = out[3], c.fc_err[e] = out[4];
        c.cost[e] = out[5], c.stress[e] = out[6];
        c.n_valid[e] = M;
        c.success[e] = reason == 0;
        c.at_bound[e] = at_bound;
        c.reason[e] = (unsigned char)reason;
    }
}

}  // namespace bpmf

using namespace bpmf;

extern "C" int bpmf_fit_spectra_dev(const double* d_average, const unsigned char* d_mask, const int* d_num_valid,
                                    const double* d_frequencies, size_t E, size_t F, int model, int phase, int weighted,
                                    double min_fraction_valid_points, double min_fraction_valid_points_below_fc,
                                    bpmf_stream_t stream_, double* d_m0, double* d_fc, double* d_mw, double* d_m0_err,
                                    double* d_fc_err, double* d_cost, double* d_stress_drop, int* d_n_valid,
                                    unsigned char* d_success, unsigned char* d_at_bound, unsigned char* d_reason)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (E == 0) return 0;
    if (!d_average || !d_mask || !d_num_valid || !d_frequencies || !d_m0 || !d_fc || !d_mw || !d_m0_err || !d_fc_err ||
        !d_cost || !d_stress_drop || !d_n_valid || !d_success || !d_at_bound || !d_reason) {
        set_error("bpmf_fit_spectra_dev: null pointer");
        return -1;
    }
    if (F == 0 || F > (size_t)FIT_MAX_FREQUENCIES || E > 0x7fffffffull / F) {
        set_error("bpmf_fit_spectra_dev: need 1 .. %d frequencies (F=%zu) and E * F < 2^31 (E=%zu)", FIT_MAX_FREQUENCIES,
                  F, E);
        return -1;
    }
    if (model < 0 || model > 1 || phase < 0 || phase > 1) {
        set_error("bpmf_fit_spectra_dev: model %d (0 Brune, 1 Boatwright), phase %d (0 P, 1 S)", model, phase);
        return -1;
    }
    // option debug.poison_output (tests): an element the kernel skips comes back as NaN / 255 / -1
    if (option(OPT_DEBUG_POISON_OUTPUT) != 0) {
        for (double* p : {d_m0, d_fc, d_mw, d_m0_err, d_fc_err, d_cost, d_stress_drop})
            BPMF_HIP_CHECK(hipMemsetAsync(p, 0xFF, E * sizeof(double), stream));
        BPMF_HIP_CHECK(hipMemsetAsync(d_n_valid, 0xFF, E * sizeof(int), stream));
        for (unsigned char* p : {d_success, d_at_bound, d_reason}) BPMF_HIP_CHECK(hipMemsetAsync(p, 0xFF, E, stream));
    }
    FitCall call{};
    call.average = d_average, call.mask = d_mask, call.num_valid = d_num_valid, call.freq = d_frequencies;
    call.m0 = d_m0, call.fc = d_fc, call.mw = d_mw, call.m0_err = d_m0_err, call.fc_err = d_fc_err, call.cost = d_cost;
    call.stress = d_stress_drop, call.n_valid = d_n_valid, call.success = d_success, call.at_bound = d_at_bound;
    call.reason = d_reason;
    call.n = model == 0 ? 2.0 : 4.0, call.crack_constant = phase == 0 ? 2.23 : 1.47;
    call.min_fraction = min_fraction_valid_points, call.min_fraction_below = min_fraction_valid_points_below_fc;
    call.F = (int)F, call.weighted = weighted ? 1 : 0;
    fit_kernel<<<dim3((unsigned)E), dim3(FIT_LANES), 0, stream>>>(call);
    BPMF_LAUNCH_CHECK();
    return 0;
}
