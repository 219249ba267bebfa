// Matched filter, full normalisation (flag BPMF_MF_NORMALIZE_FULL): the Pearson correlation of every window, i.e. the
// window mean removed.  For ANY constant c
//     sum_l (t_l - tbar)(x_l - xbar) = sum_l (t_l - tbar)(x_l - c)
//     sum_l (x_l - xbar)^2           = sum_l (x_l - c)^2 - (sum_l (x_l - c))^2 / L
// so the main kernels of mf.hip run UNCHANGED on a centred template t' = t - tbar, the day minus one constant per
// channel d' = d - c, and reciprocal norms of the centred window energies E_c = Q - P * P / L (Q, P: window sums of
// d'^2 and d').  This file is the two preparations in front of them (DESIGN.md s3 "full normalisation", s4):
//   per day     c = float32((float64 sum of the channel's FINITE samples) / N), 0 when none is finite -- it keeps P small
//               against Q, nothing else depends on it, so a NaN or +-Inf sample must not reach it: with the plain mean
//               one bad sample made d' NaN for the whole channel, windows in front of it included;
//               d'; double prefix sums of d' and d'^2 in the 1024-sample hierarchy of mf_csum_*; an integer prefix count
//               of d[n] == d[n - 1]; r_c = 1 / sqrtf((float)E_c), +Inf for a window of L equal samples (decided from the
//               count, exactly: the main kernels' r_t * r_c < 1000 guard then yields +0)
//   per batch   t' = t - float32(float64 mean), all zeros for a flat template channel (r_t = +Inf: +0 again)
#include "mf_full_api.h"
#include <cmath>

namespace bpmf {
namespace full {

constexpr size_t SUM_PART = 65536;       // samples per partial sum of a channel's mean

DayRegion carve_day(void* base, size_t N, size_t n_ch)
{
    DayRegion r;
    const size_t nq = (N + CSUM_CHUNK - 1) / CSUM_CHUNK;
    const size_t n_parts = (N + SUM_PART - 1) / SUM_PART;
    Carver c(base);
    // (the main kernels read d' through per-channel buffer descriptors: nothing outside [0, N) of a channel is fetched)
    r.dprime = c.take<float>(n_ch * N);
    r.local_p = c.take<double>(n_ch * N);
    r.tot_p = c.take<double>(n_ch * nq);
    r.off_p = c.take<double>(n_ch * nq);
    r.local_eq = c.take<int>(n_ch * N);
    r.tot_eq = c.take<int>(n_ch * nq);
    r.off_eq = c.take<int>(n_ch * nq);
    r.part = c.take<double>(n_ch * n_parts);
    r.mean = c.take<float>(n_ch);
    r.bytes = c.bytes();
    return r;
}

size_t batch_region_bytes(size_t T, size_t n_ch, size_t L) { return align_up(T * n_ch * L * sizeof(float), 256); }

// part[ch, p] = double sum of the finite samples among [p * SUM_PART, (p + 1) * SUM_PART) of channel ch (a NaN or +-Inf
// sample adds +0: the sum of a finite channel keeps its bits): every thread sums a strided share, the shares are added
// in a fixed tree (the same bits on every run).
__global__ __launch_bounds__(256) void mf_full_part_sum_kernel(const float* __restrict__ data, size_t N, size_t n_parts,
                                                               double* __restrict__ part)
{
    __shared__ double s_sum[256];
    const size_t ch = blockIdx.y, p = blockIdx.x;
    const size_t n0 = p * SUM_PART, n1 = n0 + SUM_PART < N ? n0 + SUM_PART : N;
    const float* d = data + ch * N;
    double acc = 0.0;
    for (size_t n = n0 + threadIdx.x; n < n1; n += 256) {
        const float v = d[n];
        acc = acc + ((__float_as_uint(v) & 0x7fffffffu) < 0x7f800000u ? (double)v : 0.0);
    }
    s_sum[threadIdx.x] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) s_sum[threadIdx.x] = s_sum[threadIdx.x] + s_sum[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[ch * n_parts + p] = s_sum[0];
}

// mean[ch] = float32(sum of the channel's parts / N): the sum of the finite samples over ALL N   (one thread per channel)
__global__ void mf_full_mean_kernel(const double* __restrict__ part, size_t n_ch, size_t n_parts, size_t N,
                                    float* __restrict__ mean)
{
    const size_t ch = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= n_ch) return;
    double acc = 0.0;
    for (size_t p = 0; p < n_parts; ++p) acc = acc + part[ch * n_parts + p];
    mean[ch] = (float)(acc / (double)N);
}

// One thread per 1024-sample chunk: d' = d - c (float32), the chunk-local double prefix sums of d' and d'^2, the
// chunk-local prefix count of samples equal to their predecessor (the predecessor of a chunk's first sample is the
// previous chunk's last one; sample 0 has none), and the chunk totals.
__global__ void mf_full_csum_local_kernel(const float* __restrict__ data, const float* __restrict__ mean, size_t n_ch,
                                          size_t N, size_t nq, float* __restrict__ dprime, double* __restrict__ local_p,
                                          double* __restrict__ local_q, int* __restrict__ local_eq,
                                          double* __restrict__ tot_p, double* __restrict__ tot_q, int* __restrict__ tot_eq)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_ch * nq) return;
    const size_t ch = idx / nq, q = idx % nq;
    const size_t n0 = q * CSUM_CHUNK;
    const size_t n1 = n0 + CSUM_CHUNK < N ? n0 + CSUM_CHUNK : N;
    const float* d = data + ch * N;
    float* dp = dprime + ch * N;
    double* lp = local_p + ch * N;
    double* lq = local_q + ch * N;
    int* le = local_eq + ch * N;
    const float c = mean[ch];
    // dword-aligned vector types: ch * N need not be a multiple of 4 (mf_csum_local_kernel)
    typedef float f32x4a __attribute__((ext_vector_type(4), aligned(4)));
    typedef int i32x4a __attribute__((ext_vector_type(4), aligned(4)));
    typedef double f64x2a __attribute__((ext_vector_type(2), aligned(8)));
    float prev = n0 ? d[n0 - 1] : __int_as_float(0x7fc00000);      // (a NaN equals nothing)
    double ap = 0.0, aq = 0.0;
    int ne = 0;
    size_t n = n0;
    for (; n + 4 <= n1; n += 4) {
        const f32x4a v = *(const f32x4a*)(d + n);
        f32x4a o;
        i32x4a e;
        double sp[4], sq[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float x = v[k] - c;
            const double xd = (double)x;
            o[k] = x;
            ap = ap + xd;
            aq = aq + xd * xd;           // squares are exact in double
            ne += v[k] == prev ? 1 : 0;
            prev = v[k];
            sp[k] = ap;
            sq[k] = aq;
            e[k] = ne;
        }
        *(f32x4a*)(dp + n) = o;
        *(i32x4a*)(le + n) = e;
        *(f64x2a*)(lp + n) = (f64x2a){sp[0], sp[1]};
        *(f64x2a*)(lp + n + 2) = (f64x2a){sp[2], sp[3]};
        *(f64x2a*)(lq + n) = (f64x2a){sq[0], sq[1]};
        *(f64x2a*)(lq + n + 2) = (f64x2a){sq[2], sq[3]};
    }
    for (; n < n1; ++n) {
        const float v = d[n];
        const float x = v - c;
        const double xd = (double)x;
        dp[n] = x;
        ap = ap + xd;
        aq = aq + xd * xd;
        ne += v == prev ? 1 : 0;
        prev = v;
        lp[n] = ap;
        lq[n] = aq;
        le[n] = ne;
    }
    tot_p[ch * nq + q] = ap;
    tot_q[ch * nq + q] = aq;
    tot_eq[ch * nq + q] = ne;
}

// off[ch, q] = sequential sum of tot[ch, 0 .. q-1] for the three hierarchies (one thread per channel)
__global__ void mf_full_csum_offsets_kernel(const double* __restrict__ tot_p, const double* __restrict__ tot_q,
                                            const int* __restrict__ tot_eq, size_t n_ch, size_t nq,
                                            double* __restrict__ off_p, double* __restrict__ off_q,
                                            int* __restrict__ off_eq)
{
    const size_t ch = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= n_ch) return;
    double ap = 0.0, aq = 0.0;
    int ne = 0;
    for (size_t q = 0; q < nq; ++q) {
        const size_t i = ch * nq + q;
        off_p[i] = ap;
        off_q[i] = aq;
        off_eq[i] = ne;
        ap = ap + tot_p[i];
        aq = aq + tot_q[i];
        ne += tot_eq[i];
    }
}

// r_c[ch, j] = 1 / sqrtf((float)(Q - P * P / L)), Q / P the sums of d'^2 / d' over the window [j, j + L) from the prefix
// sums (csum[n] = off[chunk(n - 1)] + local[n - 1], as mf_window_energy_kernel reads them); +Inf where the L - 1 samples
// behind the window's first all equal their predecessor.  (E_c <= 0 from rounding in a window that is NOT flat gives
// +Inf or NaN: the main kernels' guard yields 0 for both.)
__global__ void mf_full_window_norm_kernel(const double* __restrict__ local_p, const double* __restrict__ off_p,
                                           const double* __restrict__ local_q, const double* __restrict__ off_q,
                                           const int* __restrict__ local_eq, const int* __restrict__ off_eq, size_t N,
                                           size_t nq, size_t L, size_t nwin, float* __restrict__ e_d)
{
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t ch = blockIdx.y;
    if (j >= nwin) return;
    const size_t nh = j + L - 1, qh = nh / CSUM_CHUNK;
    const size_t row = ch * N, qrow = ch * nq;
    double p = off_p[qrow + qh] + local_p[row + nh];
    double q = off_q[qrow + qh] + local_q[row + nh];
    if (j > 0) {
        const size_t ql = (j - 1) / CSUM_CHUNK;
        p = p - (off_p[qrow + ql] + local_p[row + j - 1]);
        q = q - (off_q[qrow + ql] + local_q[row + j - 1]);
    }
    // samples j + 1 .. j + L - 1 that equal their predecessor
    const int n_eq = (off_eq[qrow + qh] + local_eq[row + nh]) - (off_eq[qrow + j / CSUM_CHUNK] + local_eq[row + j]);
    const float e = (float)(q - p * p / (double)L);
    e_d[ch * nwin + j] = n_eq == (int)(L - 1) ? INFINITY : 1.0f / sqrtf(e);
}

// One thread per template channel: t' = t - float32(float64 mean); a flat channel (every sample equal to the first)
// becomes exact zeros.
__global__ void mf_full_center_templates_kernel(const float* __restrict__ tmpl, size_t n_rows, size_t L,
                                                float* __restrict__ tprime)
{
    const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const float* x = tmpl + r * L;
    float* y = tprime + r * L;
    double acc = 0.0;
    bool flat = true;
    const float x0 = x[0];
    for (size_t l = 0; l < L; ++l) {
        acc = acc + (double)x[l];
        flat = flat && x[l] == x0;
    }
    const float tbar = (float)(acc / (double)L);
    for (size_t l = 0; l < L; ++l) y[l] = flat ? 0.0f : x[l] - tbar;
}

int prepare_day(const float* d_data, size_t L, size_t N, size_t n_ch, const DayRegion& day, double* local_q,
                double* tot_q, double* off_q, float* e_d, hipStream_t stream)
{
    const size_t nq = (N + CSUM_CHUNK - 1) / CSUM_CHUNK;
    const size_t n_parts = (N + SUM_PART - 1) / SUM_PART;
    const size_t nwin = N - L + 1;
    mf_full_part_sum_kernel<<<dim3((unsigned)n_parts, (unsigned)n_ch), dim3(256), 0, stream>>>(d_data, N, n_parts, day.part);
    BPMF_LAUNCH_CHECK();
    mf_full_mean_kernel<<<dim3((unsigned)((n_ch + 63) / 64)), dim3(64), 0, stream>>>(day.part, n_ch, n_parts, N, day.mean);
    BPMF_LAUNCH_CHECK();
    mf_full_csum_local_kernel<<<dim3((unsigned)((n_ch * nq + 63) / 64)), dim3(64), 0, stream>>>(
        d_data, day.mean, n_ch, N, nq, day.dprime, day.local_p, local_q, day.local_eq, day.tot_p, tot_q, day.tot_eq);
    BPMF_LAUNCH_CHECK();
    mf_full_csum_offsets_kernel<<<dim3((unsigned)((n_ch + 63) / 64)), dim3(64), 0, stream>>>(
        day.tot_p, tot_q, day.tot_eq, n_ch, nq, day.off_p, off_q, day.off_eq);
    BPMF_LAUNCH_CHECK();
    mf_full_window_norm_kernel<<<dim3((unsigned)((nwin + 255) / 256), (unsigned)n_ch), dim3(256), 0, stream>>>(
        day.local_p, day.off_p, local_q, off_q, day.local_eq, day.off_eq, N, nq, L, nwin, e_d);
    BPMF_LAUNCH_CHECK();
    return 0;
}

int prepare_templates(const float* d_templates, size_t n_rows, size_t L, float* tprime, hipStream_t stream)
{
    mf_full_center_templates_kernel<<<dim3((unsigned)((n_rows + 63) / 64)), dim3(64), 0, stream>>>(d_templates, n_rows, L,
                                                                                                   tprime);
    BPMF_LAUNCH_CHECK();
    return 0;
}

}  // namespace full
}  // namespace bpmf
